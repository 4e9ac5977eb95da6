"""Batches that steer the waves of the Panda row kernels onto a CHOSEN solver path (tests only).

Core::step for the 16-lane shape picks its sweep code per wave from the union of the row sets of the wave's four envs
(csrc/pbre_core.hpp, "16-lane rows"): the robot-only chain (with nine further copies, one per joint, for a wave with exactly one joint
at a limit), the zipped two-chain sweeps (three instantiations by robot-object slot mask, the robot-table friction rows riding along
with the next sweep's motor rows -- `e_zip` -- or not), and the loops with per-slot tests.  Which envs share a wave is known exactly in
two places:

  k_step      (F_FORCE_GENERAL)  env i is row i % 16 of block i / 16: envs 4k .. 4k+3 share a wave
  k_row_list  (F_COMPLEX_ROWS)   uncoupled complex envs fill the rows of an item in list order: with at most four of them in the batch
                                 they share wave 0 whatever order the atomics produce; a coupled env has a wave to itself

Everything here runs on the CPU from the oracle alone: single-env states by row signature, waves built from them, the wave's pattern
by the rule above, the assertion that a family of batches contains every pattern it is meant to, and the pre-filter that leaves only
states the oracle itself calls well conditioned (so that the comparisons of tests/test_*_row_paths.py skip nothing).

A FAMILY is a list of VARIANT batches of one size.  Env 4w (k_step) of every variant is the same PROBE state with the same action; the
three wave-mates differ from variant to variant, so the probe's wave takes another path.  The probe's state record and output row
must not depend on that, bit for bit.
"""
import functools

import numpy as np

import orc
import parity
import scenarios

NJ = 9
SEED = 20240917


class FixedActions:
    """Stands in for the rng of parity.check_single_steps: the batch's own actions instead of fresh random ones."""

    def __init__(self, a):
        self.a = np.asarray(a, np.float32)

    def uniform(self, lo, hi, shape):
        assert tuple(shape) == self.a.shape
        return self.a.copy()


class Lab:
    """fp64 and fp32 oracle with the same settings, the reset state, the joint limits."""

    def __init__(self, panda, no_object=False, phys=None):
        self.panda, self.no_object, self.phys = panda, no_object, dict(phys or {})
        self.task = 0 if no_object else 1
        self.ora, self.ora32 = (self._oracle(f32) for f32 in (False, True))
        self.base = self.ora.batch_reset(1)[0][0]
        self.lo, self.hi = scenarios.joint_limits(self.ora)

    def _oracle(self, f32):
        o = orc.Oracle(self.panda["table"], f32=f32, task=self.task)
        o.task.obj_pose_rnd_std, o.task.tg_pose_rnd_std = 0.05, (0.0 if self.no_object else 0.2)
        if self.no_object:
            o.params.flags = orc.F_NO_OBJECT
        for k, v in self.phys.items():
            setattr(o.params, k, v)
        return o

    def engine(self, Engine, lib, n, flags):
        from pybullet_robot_envs import _capi
        return Engine(self.panda["table"], task=self.task, num_envs=n, lib=lib, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.0 if self.no_object else 0.2,
                      flags=flags | (_capi.F_NO_OBJECT if self.no_object else 0), **({"phys": self.phys} if self.phys else {}))

    # ---- row signature of one state, from the oracle alone
    def signature(self, s):
        """(joints at a limit, robot-object contacts, robot-table contacts, object-table contacts) of the fp32 state s"""
        s = np.asarray(s, np.float32).astype(np.float64)
        _, info = self.ora.sim_step(s, s[:NJ].copy(), np.full(NJ, 0.1), np.full(NJ, 1.0))
        t = [info.type[k] for k in range(info.ncontacts)]
        lim = frozenset(j for j in range(NJ) if s[j] - self.lo[j] <= 0 or self.hi[j] - s[j] <= 0)       # the oracle's own test (limit rows)
        return lim, t.count(1), t.count(2), t.count(0)


def wave_pattern(sigs, no_object):
    """The path Core::step takes for a wave of envs with these signatures (pbre_core.hpp: robot_only / ot_all / with_ro, ro_bits, rt_bits,
    lim_bits, e_zip).  Robot-object and robot-table slots fill in rank order from slot 0, so a count c is the slot mask (1 << c) - 1 and the
    wave's mask is that of its largest count."""
    lim = frozenset().union(*[s[0] for s in sigs])
    nro, nrt, not_ = max(s[1] for s in sigs), max(s[2] for s in sigs), max(s[3] for s in sigs)
    rt = "rt%d" % (nrt > 0)
    if no_object or (nro == 0 and not_ == 0):
        lj = "none" if not lim else ("LJ%d" % min(lim) if len(lim) == 1 else "multi")
        return "ro/%s/%s" % (lj, rt)
    ot = "ot4" if not_ == 4 else "otlt4"
    lm = "lim%d" % (len(lim) > 0)
    if nro > 0 or not_ == 4:
        return "zip/nro%s/%s/%s/%s%s" % (("0", "1", "2", "3+", "3+")[nro], lm, rt, ot, "/e_zip" if nrt > 0 and not lim else "")
    return "loops/%s/%s/%s" % (lm, rt, ot)


def required_patterns(kind):
    if kind == "ro":
        return (["ro/none/rt0", "ro/none/rt1", "ro/multi/rt0", "ro/multi/rt1"] + ["ro/LJ%d/rt%d" % (j, r) for j in range(NJ) for r in (0, 1)])
    req = []
    for lm in (0, 1):
        for rt in (0, 1):
            ez = "/e_zip" if rt and not lm else ""
            req += ["zip/nro%s/lim%d/rt%d/ot4%s" % (k, lm, rt, ez) for k in ("0", "1", "2", "3+")]
            req += ["zip/nro1/lim%d/rt%d/otlt4%s" % (lm, rt, ez), "loops/lim%d/rt%d/otlt4" % (lm, rt)]
    return req


# ---- pools of single-env states by signature
class Pools:
    def __init__(self, lab, seed):
        self.lab, self.rng = lab, np.random.default_rng(seed)
        self.pool, self.used = {}, {}

    def _free_arm(self):
        lab, rng = self.lab, self.rng
        s = lab.base.copy()
        q = scenarios.HOME + rng.normal(0, 0.25, NJ)
        q[7:] = rng.uniform(0.005, 0.035, 2)
        s[:NJ] = np.clip(q, lab.lo + 0.05 * (lab.hi - lab.lo), lab.hi - 0.05 * (lab.hi - lab.lo))
        s[16:25] = rng.normal(0, 0.3, NJ)
        return s

    def _past_limit(self, s, j, side):
        """joint j 2 - 20 mm (arm; rad for the revolute joints) or 0.5 - 3 mm (fingers) PAST its limit -- never on it: fp32 rounding of the
        limit would flip the row"""
        pen = self.rng.uniform(0.002, 0.02) if j < 7 else self.rng.uniform(0.0005, 0.003)
        s[j] = self.lab.lo[j] - pen if side == 0 else self.lab.hi[j] + pen

    def _tip(self, s):
        """the cube tipped onto an edge: fewer than four object-table contacts"""
        ang = np.deg2rad(self.rng.uniform(15.0, 30.0))
        s = s.copy()
        s[12:16] = [np.sin(ang / 2), 0, 0, np.cos(ang / 2)]
        s[11] = self.lab.base[11] + 0.025 * (np.sin(ang) + np.cos(ang) - 1.0) + self.rng.uniform(-0.0005, 0.0003)
        return s

    def _make(self, name):
        """candidates for pool `name` (not yet checked against its signature)"""
        lab, rng, P = self.lab, self.rng, self.lab.panda
        kind = name.split(":")[0]
        tipped = name.endswith(":tip")
        if kind == "free":
            S = [self._free_arm() for _ in range(8)]
        elif kind == "lim":               # lim:<j>:<side>
            _, j, side = name.split(":")[:3]
            S = [self._free_arm() for _ in range(6)]
            for s in S:
                self._past_limit(s, int(j), int(side))
        elif kind == "lim2":              # two joints of one env at a limit
            S = [self._free_arm() for _ in range(6)]
            for s in S:
                j = int(rng.integers(0, 7))
                self._past_limit(s, j, int(rng.integers(0, 2)))
                self._past_limit(s, (j + int(rng.integers(1, 7))) % 7, int(rng.integers(0, 2)))
        elif kind == "table":
            S = list(scenarios.table_contact_states(lab.ora, P["model"], P["spheres"], lab.base, 8, rng))
        elif kind in ("ro1", "ro2"):
            S = list(scenarios.object_contact_states(lab.ora, P["model"], P["spheres"], lab.base, 12, rng))
        elif kind == "ro3":
            S = list(scenarios.multi_sphere_object_states(lab.ora, P["model"], P["spheres"], lab.base, 6, rng, want=3))
        else:
            raise KeyError(name)
        if tipped:
            S = [self._tip(s) for s in S]
        return [np.asarray(s, np.float32) for s in S]

    def _fits(self, name, sig):
        lim, nro, nrt, not_ = sig
        kind = name.split(":")[0]
        tipped = name.endswith(":tip")
        if not self.lab.no_object:
            if tipped and not 0 < not_ < 4:
                return False
            if not tipped and kind in ("free", "lim", "lim2", "table") and not_ != 4:
                return False
        if kind == "free":
            return not lim and nro == 0 and nrt == 0
        if kind == "lim":
            return lim == {int(name.split(":")[1])} and nro == 0 and nrt == 0
        if kind == "lim2":
            return len(lim) == 2 and nro == 0 and nrt == 0
        if kind == "table":
            return not lim and nro == 0 and nrt > 0
        want = {"ro1": (1,), "ro2": (2,), "ro3": (3, 4)}[kind]
        return not lim and nro in want and nrt == 0 and not_ < 4         # (the cube is held up against the hand: off the table)

    def take(self, name):
        """the next unused (state, action, signature) of pool `name`"""
        lst = self.pool.setdefault(name, [])
        k = self.used.get(name, 0)
        tries = 0
        while k >= len(lst):
            tries += 1
            assert tries < 200, "no state with the signature of pool %r" % name
            for s in self._make(name):
                sig = self.lab.signature(s)
                if self._fits(name, sig):
                    lst.append((s, self.rng.uniform(-1, 1, 7).astype(np.float32), sig))
        self.used[name] = k + 1
        return lst[k]


def flagged(lab, S, A, tol=None):
    """Envs that parity.check_single_steps(skip_ambiguous=True, ora32=...) would skip in the batch (S, A): a contact candidate within 3 um of
    the margin (parity.ambiguous_envs), or a result that moves by more than half the bounds when the fp64 oracle's input is perturbed at the
    fp32 rounding level or its fp32 build runs instead -- the same probe, with the same perturbations (they depend on the batch size and the
    env's position only).  Oracle only: no engine is involved."""
    tt = parity.TOL_CONTACT if tol is None else tol
    s32 = np.asarray(S, np.float32)
    s64 = s32.astype(np.float64)
    n = len(s32)
    bad = parity.ambiguous_envs(lab.ora, s64, A)
    so, out = lab.ora.batch_step(s64, A)
    prng = np.random.default_rng(12345)
    trials = [lab.ora32.batch_step(s32, A)]
    for _ in range(4):
        sp = s32.astype(np.float64)
        sp[:, :31] *= 1.0 + prng.uniform(-2e-7, 2e-7, (n, 31))
        trials.append(lab.ora.batch_step(sp, A))
    for s_f, o_f in trials:
        qf = quantities_per_env(np.asarray(s_f, np.float64), so, np.asarray(o_f[:, :-2], np.float64), out)
        for k, v in qf.items():
            if k in tt:
                bad |= v > 0.5 * tt[k]
    return bad


def quantities_per_env(se, so, ob, out):
    """parity.panda_quantities env by env: the same quantities, one value per env instead of the batch's maximum"""
    o = out[:, :-2]
    m = lambda x: np.abs(x).max(axis=1)
    sgn = np.sign((se[:, 12:16] * so[:, 12:16]).sum(1, keepdims=True))
    q = {"q": m(se[:, 0:9] - so[:, 0:9]), "qd": m(se[:, 16:25] - so[:, 16:25]), "obj_pos": m(se[:, 9:12] - so[:, 9:12]),
         "obj_quat": m(se[:, 12:16] * sgn - so[:, 12:16]), "obj_v": m(se[:, 25:28] - so[:, 25:28]), "obj_w": m(se[:, 28:31] - so[:, 28:31]),
         "obs_ee_pos": m(ob[:, 0:3] - o[:, 0:3]), "obs_ee_eul": parity.angdiff(ob[:, 3:6], o[:, 3:6]).max(axis=1), "obs_ee_vel": m(ob[:, 6:9] - o[:, 6:9]),
         "obs_q": m(ob[:, 9:18] - o[:, 9:18]), "obs_obj_pos": m(ob[:, 18:21] - o[:, 18:21]), "obs_obj_eul": parity.angdiff(ob[:, 21:24], o[:, 21:24]).max(axis=1),
         "obs_rel_pos": m(ob[:, 24:27] - o[:, 24:27]), "obs_rel_eul": parity.angdiff(ob[:, 27:30], o[:, 27:30]).max(axis=1)}
    if ob.shape[1] > 30:
        q["obs_target"] = m(ob[:, 30:33] - o[:, 30:33])
    return q


class Family:
    """variants[v] = (S [n, STATE] float32, A [n, 7] float32); names[v][e] = the pool env e was drawn from, sigs[v][e] its row signature;
    patterns[v][w] = pattern of wave w; probes = env indices whose state and action are the same in every variant"""

    def __init__(self, kind, lab, flags, wave_of):
        self.kind, self.lab, self.flags, self.wave_of = kind, lab, flags, wave_of
        self.variants, self.sigs, self.patterns, self.probes, self.names = [], [], [], [], []

    @property
    def n(self):
        return len(self.variants[0][0])

    def all_patterns(self):
        return set(p for pv in self.patterns for p in pv if p)


def _build(kind, lab, flags, plan, seed, wave_of):
    """plan[v][w] = pool names of the envs of wave w in variant v (k_step families: four per wave; the first, marked *, is the probe and is
    the same in every variant).  Draws the states -- an env position that has the same pool name in several variants gets the same state
    in all of them --, re-draws every env that `flagged` objects to and computes the patterns."""
    pools = Pools(lab, seed)
    nv = len(plan)
    slots = [[nm for wave in pv for nm in wave] for pv in plan]
    n = len(slots[0])
    assert all(len(s) == n for s in slots)
    probes = [e for e in range(n) if all(slots[v][e] == slots[0][e] and slots[0][e].startswith("*") for v in range(nv))]
    at = {}                # (env position, pool name) -> (state, action, signature)

    def batch(v):
        return [at[(e, slots[v][e])] for e in range(n)]

    for v in range(nv):
        for e in range(n):
            if (e, slots[v][e]) not in at:
                at[(e, slots[v][e])] = pools.take(slots[v][e].lstrip("*"))
    for rnd in range(40):
        again = set()
        for v in range(nv):
            cur = batch(v)
            S = np.array([c[0] for c in cur]); A = np.array([c[1] for c in cur])
            for e in np.nonzero(flagged(lab, S, A))[0]:
                again.add((int(e), slots[v][e]))
        if not again:
            break
        for key in sorted(again):
            at[key] = pools.take(key[1].lstrip("*"))
    else:
        raise AssertionError("family %r: still ill-conditioned states after 40 rounds of re-drawing" % kind)
    cur = [batch(v) for v in range(nv)]
    fam = Family(kind, lab, flags, wave_of)
    fam.probes = probes
    for v in range(nv):
        fam.variants.append((np.array([c[0] for c in cur[v]]), np.array([c[1] for c in cur[v]])))
        fam.sigs.append([c[2] for c in cur[v]])
        fam.names.append([s.lstrip("*") for s in slots[v]])
    return fam


def _k_step_patterns(fam):
    for v in range(len(fam.variants)):
        sg = fam.sigs[v]
        fam.patterns.append([wave_pattern(sg[4 * w:4 * w + 4], fam.lab.no_object) for w in range(len(sg) // 4)])


@functools.lru_cache(maxsize=None)
def _lab(panda_key, no_object, phys):
    return Lab(_PANDA[panda_key], no_object, dict(phys))


_PANDA = {}


def lab_of(panda, no_object=False, phys=()):
    _PANDA[id(panda)] = panda
    return _lab(id(panda), no_object, tuple(sorted(dict(phys).items())))


@functools.lru_cache(maxsize=None)
def _family(panda_key, kind):
    return _FAMILIES[kind](_PANDA[panda_key])


def family(panda, kind):
    """cached: the states and the oracle's verdicts are computed once per process"""
    _PANDA[id(panda)] = panda
    return _family(id(panda), kind)


def other(j):
    return (j + 3) % 7


def family_ro(panda, phys=(), kind="ro", seed=SEED + 1):
    """k_step, F_FORCE_GENERAL | F_NO_OBJECT: every wave is `robot_only`.  Probes: joint j past its lower / upper limit for j = 0..8, and some
    free, table-contact and two-limit envs.  Variants -- the probe's three wave-mates are
        0  free envs                                          (limit probe: the LJ = j copy, no robot-table rows)
        1  envs with robot-table contacts                     (the LJ = j copy with the robot-table rows)
        2  an env with ANOTHER joint at its limit + two free  (two limit joints in the wave: the loop with per-joint tests, LJ = -1)
        3  an env with the SAME joint at its limit + two free (limit probes: one limit joint from two groups, the LJ = j copy again)"""
    from pybullet_robot_envs import _capi
    lab = lab_of(panda, True, phys)
    probes = ["*lim:%d:%d" % (j, side) for j in range(NJ) for side in (0, 1)] + ["*free"] * 2 + ["*table"] * 3 + ["*lim2"] * 2
    plan = [[], [], [], []]
    for k, p in enumerate(probes):
        j = int(p.split(":")[1]) if p.startswith("*lim:") else k % NJ
        plan[0].append([p, "free", "free", "free"])
        plan[1].append([p, "table", "table", "table"])
        plan[2].append([p, "lim:%d:%d" % (other(j), k % 2), "free", "free"])
        plan[3].append([p, "free", "lim:%d:%d" % (j, (k + 1) % 2), "free"] if p.startswith("*lim:") else [p, "lim:%d:0" % j, "lim:%d:1" % other(j), "table"])
    fam = _build(kind, lab, _capi.F_FORCE_GENERAL, plan, seed, "k_step")
    _k_step_patterns(fam)
    return fam


def _zip_plan(keep):
    probes = ["*ro1"] * 3 + ["*ro2"] * 3 + ["*ro3"] * 3 + ["*free"] * 2 + ["*table"] * 2 + ["*free:tip"] * 2 + ["*ro1"]
    variants = [(o, l, t, tip) for tip in (0, 1) for l in (0, 1) for t in (0, 1) for o in ((0, 1) if not tip else (0,))]
    variants = [key for key in variants if keep is None or key in keep]
    plan = []
    for (o, l, t, tip) in variants:
        pv = []
        for k, p in enumerate(probes):
            sfx = ":tip" if tip else ""
            oth = "ro2" if p == "*ro1" else "ro1"          # (a one-contact probe beside a two-contact mate: the wave's slot mask is 3)
            j = (2 * k + 1) % NJ
            pv.append([p, oth if o else "free" + sfx, ("lim:%d:%d" % (j, k % 2)) + sfx if l else "free" + sfx, "table" + sfx if t else "free" + sfx])
        plan.append(pv)
    return plan, variants


def family_zip(panda, phys=(), kind="zip", seed=SEED + 2, keep=None):
    """k_step, F_FORCE_GENERAL, with the cube.  Probes: one / two / three-or-four robot-object contacts (the cube held against the hand, off
    the table), a free arm over a resting cube, an arm on the table, a free arm over a cube tipped onto an edge.  Variants: the wave-mates are
    free envs, or one of them has (o) another number of robot-object contacts, (l) a joint at its limit, (t) robot-table contacts, and
    (tip) all of them have tipped cubes -- with a probe whose cube is off the table the wave then uses fewer than four object-table slots.
    keep: only these variants (o, l, t, tip)."""
    from pybullet_robot_envs import _capi
    lab = lab_of(panda, False, phys)
    plan, variants = _zip_plan(keep)
    fam = _build(kind, lab, _capi.F_FORCE_GENERAL, plan, seed, "k_step")
    fam.variant_keys = variants
    _k_step_patterns(fam)
    return fam


CLAMP = (("max_motor_impulse", 0.004),)


def family_clamp(panda):
    """the zipped-chain family with motors that reach their impulse bound (max_motor_impulse 0.004, as in
    test_two_chain_sweeps_are_bit_identical): the clamping motor stages bind.  Four of its variants."""
    return family_zip(panda, CLAMP, "clamp", SEED + 3, keep=((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 1, 0), (0, 0, 1, 1)))


def family_ro_clamp(panda):
    """the robot-only family with motors that reach their impulse bound.  A position motor with PyBullet's default force undoes a limit row's
    impulse on its joint in the same sweep (both rows act through the same column of M^-1, and the motor row comes last in the last sweep),
    so with unbounded motors a limit row that is missing or applied to the wrong joint changes the result by rounding only: check (b) sees
    it, the comparison with the oracle cannot.  With bounded motors the limit rows decide where the joint goes, and the oracle sees them."""
    return family_ro(panda, CLAMP, "ro_clamp", SEED + 4)


ROWS_N = 64
ROWS_PROBE, ROWS_MATES, ROWS_COUPLED = 5, (22, 43, 60), 33


def family_rows(panda):
    """F_COMPLEX_ROWS, 64 envs: env 5 is the probe (an uncoupled complex env: a joint past its limit, j = 0..8, or robot-table contacts),
    envs 22 / 43 / 60 its up to three uncoupled wave-mates -- at most four uncoupled complex envs in the batch: wave 0 of k_row_list's only
    item whatever order the atomics produce --, env 33 a coupled env (robot-object contacts: a wave to itself), all others simple.  The row
    waves leave the object to the object wave, so the uncoupled wave sweeps the robot-only chain.  One variant = one step = one pattern:
        0  the probe alone            1  + a table-contact env            2  + another limit joint and a table-contact env
        3  + three mates: the same joint at its limit, another joint, robot-table contacts"""
    from pybullet_robot_envs import _capi
    lab = lab_of(panda, False)
    probes = ["lim:%d:%d" % (j, j % 2) for j in range(NJ)] + ["table"]
    fams = []
    for k, p in enumerate(probes):        # one _build per probe: its four variants share the probe and the coupled env
        j = int(p.split(":")[1]) if p.startswith("lim") else 3
        plan = []
        for mates in ([], ["table"], ["lim:%d:1" % other(j), "table"], ["lim:%d:%d" % (j, (j + 1) % 2), "lim:%d:0" % other(j), "table"]):
            names = ["free"] * ROWS_N
            names[ROWS_PROBE] = "*" + p
            for pos, nm in zip(ROWS_MATES, mates):
                names[pos] = nm
            names[ROWS_COUPLED] = "*" + ("ro1", "ro2", "ro3")[k % 3]
            plan.append([names])
        f = _build("rows", lab, _capi.F_COMPLEX_ROWS, plan, SEED + 10 + k, "k_row_list")
        for v in range(4):
            sg = f.sigs[v]
            unc = [sg[e] for e in (ROWS_PROBE,) + ROWS_MATES if sg[e][0] or sg[e][2]]
            f.patterns.append([wave_pattern(unc, True), wave_pattern([sg[ROWS_COUPLED]], False)])
            for e in range(ROWS_N):        # every other env is simple
                assert e in (ROWS_PROBE, ROWS_COUPLED) + ROWS_MATES or sg[e] == (frozenset(), 0, 0, 4)
        fams.append(f)
    return fams


_FAMILIES = {"ro": family_ro, "ro_clamp": family_ro_clamp, "zip": family_zip, "clamp": family_clamp, "rows": family_rows}


def assert_coverage(fam):
    have = fam.all_patterns()
    missing = [p for p in required_patterns("ro" if fam.kind.startswith("ro") else "zip") if p not in have]
    if fam.kind == "clamp":
        missing = [p for p in ("zip/nro1/lim0/rt0/ot4", "zip/nro2/lim0/rt0/ot4", "zip/nro1/lim1/rt1/ot4") if p not in have]
    assert not missing, "family %r lacks the wave patterns %r (has %r)" % (fam.kind, missing, sorted(have))
    if fam.kind in ("zip", "clamp"):
        # the union rule: a one-contact env and a two-contact env in one wave (slot masks 1 and 3, the wave's is 3)
        assert any({1, 2} <= set(s[1] for s in sg[4 * w:4 * w + 4]) for sg in fam.sigs for w in range(len(sg) // 4))
    if fam.kind.startswith("ro"):
        # one limit joint from two groups of the wave / two limit joints in one env
        assert any(sum(1 for s in sg[4 * w:4 * w + 4] if s[0]) == 2 and pv[w].startswith("ro/LJ") for sg, pv in zip(fam.sigs, fam.patterns) for w in range(len(pv)))
        assert any(any(len(s[0]) == 2 for s in sg[4 * w:4 * w + 4]) for sg in fam.sigs for w in range(len(sg) // 4))
    # every probe's wave takes more than one path over the variants
    for e in fam.probes:
        assert len(set(pv[e // 4] for pv in fam.patterns)) > 1, (e, [pv[e // 4] for pv in fam.patterns])


def assert_rows_coverage(fams):
    """the F_COMPLEX_ROWS batches: every LJ copy with and without robot-table rows, the loop with per-joint tests, no limit at all, one to
    four uncoupled envs, and a coupled env with one / two / three-or-four robot-object contacts"""
    unc = set(pv[0] for f in fams for pv in f.patterns)
    cpl = set(pv[1] for f in fams for pv in f.patterns)
    missing = [p for p in ["ro/LJ%d/rt%d" % (j, r) for j in range(NJ) for r in (0, 1)] + ["ro/multi/rt1", "ro/none/rt1"] if p not in unc]
    missing += [p for p in ["zip/nro%s/lim0/rt0/otlt4" % k for k in ("1", "2", "3+")] if p not in cpl]
    assert not missing, "the row-list batches lack the wave patterns %r" % missing
    counts = set(sum(1 for e in (ROWS_PROBE,) + ROWS_MATES if sg[e][0] or sg[e][2]) for f in fams for sg in f.sigs)
    assert counts == {1, 2, 3, 4}, counts
    for f in fams:
        assert f.probes == [ROWS_PROBE, ROWS_COUPLED] and len(set(pv[0] for pv in f.patterns)) > 1


def complex_envs(fam, v):
    """how many envs of variant v the engine must class as complex (a joint at a limit, or a robot contact)"""
    return sum(1 for s in fam.sigs[v] if s[0] or s[1] or s[2])


# ---- the checks (engine = the HIP library or the host emulation)
def check_oracle(fam, eng, v, report=None):
    """(a) one step of variant v from identical fp32 states against the oracle: TOL_CONTACT, nothing skipped, no outlier"""
    S, A = fam.variants[v]
    try:
        rep = parity.check_single_steps(eng, fam.lab.ora, S, FixedActions(A), steps=1, tol=parity.TOL_CONTACT, skip_ambiguous=True, max_skip=0.1,
                                        ora32=fam.lab.ora32, max_outliers=0, report=report)
    except AssertionError as ex:      # say WHICH envs: the state the engine is left in is the step's result
        so, _ = fam.lab.ora.batch_step(S.astype(np.float64), A)
        se = np.asarray(eng.get_state(), np.float64)
        off = [e for e in range(len(S)) if np.abs(se[e, :NJ] - so[e, :NJ]).max() > parity.TOL_CONTACT["q"] or np.abs(se[e, 16:25] - so[e, 16:25]).max() > parity.TOL_CONTACT["qd"]]
        raise AssertionError("%s -- %s variant %d, envs beyond the q / qd bounds: %r" % (ex, fam.kind, v, [(e, fam.names[v][e], fam.patterns[v][0 if fam.wave_of == "k_row_list" else e // 4]) for e in off]))
    assert rep["skipped_ambiguous"] == 0, "the pre-filter left %d ill-conditioned states in" % rep["skipped_ambiguous"]
    if parity.MEASURE:       # (PBRE_PARITY_MEASURE=1: the record of the margin under TOL_CONTACT, profiles/r09_row_paths.json -- no bound is derived from it)
        import json
        print("ROW_PATHS " + json.dumps({"family": fam.kind, "variant": v, "kernel": fam.wave_of, "envs": len(S), "patterns": sorted(set(fam.patterns[v])),
                                         "worst": dict((k, float("%.3g" % x)) for k, x in rep["worst"].items())}))
    return rep


def step_bits(eng, S, A):
    eng.set_state(S)
    ob, rw, dn = eng.step(A)
    st = eng.get_state()
    row = np.concatenate([np.asarray(ob, np.float32), np.asarray(rw, np.float32).reshape(len(S), -1), np.asarray(dn, np.float32).reshape(len(S), -1)], 1)
    return np.ascontiguousarray(st, np.float32).view(np.uint32).copy(), np.ascontiguousarray(row).view(np.uint32).copy()


def check_path_independence(fam, eng, sweeps=False):
    """(b) the probes' state records and output rows (and, with the residual exit on, sweep counts) are bit-identical over the variants.
    Returns, per probe, the patterns its wave took."""
    ref = None
    for v, (S, A) in enumerate(fam.variants):
        st, row = step_bits(eng, S, A)
        sw = eng.get_sweeps().copy() if sweeps else None
        if ref is None:
            ref = (st, row, sw)
            continue
        for e in fam.probes:
            w = 0 if fam.wave_of == "k_row_list" else e // 4
            ctx = "env %d (%s): variant 0 wave %s, variant %d wave %s" % (e, fam.names[0][e], fam.patterns[0][min(w, len(fam.patterns[0]) - 1)], v,
                                                                       fam.patterns[v][min(w, len(fam.patterns[v]) - 1)])
            assert np.array_equal(ref[0][e], st[e]), "state record differs with the wave's path: " + ctx
            assert np.array_equal(ref[1][e], row[e]), "output row differs with the wave's path: " + ctx
            if sweeps:
                assert ref[2][e] == sw[e], "sweep count differs with the wave's path: " + ctx


def check_residual_exit(fam, eng, v, thr=1e-7, max_flip=0.05):
    """(c) variant v with solver_residual_threshold = thr in engine and oracle: the assertions of parity.check_residual_threshold on the sweep
    counts (equal to the oracle's but for a bounded fraction of one-sweep flips, never more than two sweeps apart) and on the results
    (TOL_CONTACT where the counts agree, TOL_RT_FLIP where they do not)."""
    S, A = fam.variants[v]
    ora = fam.lab.ora
    n = len(S)
    eng.set_physics(solver_residual_threshold=thr)
    ora.params.solver_residual_threshold = thr
    try:
        eng.set_state(S)
        ob, rw, dn = eng.step(A)
        se, sw = eng.get_state(), eng.get_sweeps()
        so, out, used, _ = ora.batch_step_sweeps(S.astype(np.float64), A)
    finally:
        ora.params.solver_residual_threshold = 0.0
        eng.set_physics(solver_residual_threshold=0.0)
    iters = int(ora.params.solver_iters)
    assert sw.min() >= 1 and sw.max() <= iters
    same, flip = sw == used, sw != used
    assert flip.sum() <= max(1, int(max_flip * n)), "exit sweeps differ in %d of %d envs" % (flip.sum(), n)
    assert not flip.any() or np.abs(sw[flip].astype(int) - used[flip]).max() <= 2
    assert (used < iters).any(), "the residual test never fired: nothing tested"
    assert (dn != out[:, -1]).sum() <= max(1, n // 50)
    worst = parity.panda_quantities(se[same], so[same], ob[same], out[same])
    parity.assert_within(worst, parity.TOL_CONTACT, "(%s variant %d, residual threshold %g: %d envs with equal sweep counts)" % (fam.kind, v, thr, same.sum()))
    if flip.any():
        parity.assert_within(parity.panda_quantities(se[flip], so[flip], ob[flip], out[flip]), parity.TOL_RT_FLIP, "(%d envs a sweep apart)" % flip.sum())
    return {"flips": int(flip.sum()), "early": int((used < iters).sum()), "worst": worst}
