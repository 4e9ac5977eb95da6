"""The constraint solver at sweep counts other than 150 (tests only; see DESIGN.md section 2, "Sweep counts other than 150").

pbre_physics.solver_iters is a runtime parameter, and in the kernels it is more than a loop bound: the simple class takes the motors' closed
form (a matrix power by binary powering of iters / 2) only at even counts >= 4, the object block's closed form and the closed form of the
residual exit only at even counts >= PBRE_OC_K + 32, and every two-sweeps-per-trip loop of the row kernels leaves through
`if (it + 1 >= P.iters) break` at odd counts.  The checks here run the existing comparisons -- closed forms against Bullet's sequential rows,
the engines against the fp64 oracle, the per-wave path families of tests/row_paths.py, the residual exit -- at counts on either side of
each of these conditions, with the existing tolerances.

Every engine is created and reset at the default count and then switched with set_physics(solver_iters=k) (parity.set_solver_iters, which
also switches the oracle: otherwise that silently stays at 150); the families of row_paths, which never reset, are created at k through
Engine(phys=...).  The one bound that is not an existing one is the rule for a resting cube's angular velocity at counts below the object
closed form's threshold (check_free_steps); the odd-count exit of the lane-group engines is checked at 1 and 3 sweeps without a
tolerance on the engine (assert_odd_exit)."""
import functools
import json

import numpy as np

import orc
import parity
import row_paths
from pybullet_robot_envs import _capi

OC_K = 22                       # PBRE_OC_K (csrc/pbre_fast.hpp): the object block's closed form and the residual exit's need iters >= OC_K + 32
OC_MIN = OC_K + 32

CLOSED_COUNTS = [2, 3, 4, 5, 6, 8, 10, 50, 51, 52, 54, 56, 150, 300, 1000]
FREE_COUNTS = [1, 2, 3, 4, 5, 6, 8, 21, 50, 51, 52, 53, 54, 55, 56, 150, 151, 300, 400]
CONTACT_COUNTS = [1, 2, 3, 50, 51, 300]
FAMILY_COUNTS = [3, 51, 300]
FAMILY_RT_COUNTS = [51, 300]
RT_COUNTS = [50, 51, 52, 53, 54, 56, 100, 300]      # (51, 53: the explicit RT rows of the simple class leave at an odd cap)
GROUP_COUNTS = [50, 51, 300]

_CACHE = {}


def cached(key, make):
    """engines (and what was computed once for them) shared by the cases of a parametrised test: one reset, at the default count"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def motor_closed_taken(k):
    return k >= 4 and k % 2 == 0


# ---------------------------------------------------------------------------------------------- A1
def closed_form_engines(Engine, lib, table, n):
    kw = dict(task=1, num_envs=n, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, lib=lib)
    c = Engine(table, **kw)
    s = Engine(table, flags=_capi.F_SEQ_MOTORS | _capi.F_SEQ_OBJECT, **kw)
    c.reset(); s.reset()
    rng = np.random.default_rng(23)
    st, kind = parity.object_block_states(c.get_state()[0], rng, n)
    st[:, 16:25] = rng.normal(0, 0.3, (n, 9)).astype(np.float32)
    return c, s, st


def check_closed_forms(c, s, st, k, steps=4, seed=29):
    """Fast::motor_closed and Fast::obj_closed against Bullet's sequential rows (PBRE_F_SEQ_MOTORS | PBRE_F_SEQ_OBJECT), fp32 on both sides,
    at k sweeps: cubes at rest, sliding, spinning, dropped, tilted, tumbling, pressed (parity.object_block_states) under arms that move.
    Odd counts and counts below 4: no closed form may be taken, so state records and output rows are bit-identical.  Even counts >= 4:
    within a quarter of the single-step bounds (half for the object's twist, as in parity.check_closed_form_object_rows), and NOT
    bit-identical in every env-step: the closed form was taken."""
    n = len(st)
    rng = np.random.default_rng(seed)
    for e in (c, s):
        parity.set_solver_iters(e, k)
    c.set_state(st)
    worst, exact = {}, 0
    for t in range(steps):
        a = (rng.uniform(-1, 1, (n, 7)) * 0.3).astype(np.float32)
        s.set_state(c.get_state())
        (obc, rwc, dnc), (obs_, rws, dns) = c.step(a), s.step(a)
        sc, ss = c.get_state(), s.get_state()
        assert c.kernel_info()[5] == 0 and s.kernel_info()[5] == 0, "an env left the simple class"
        rc = np.concatenate([obc, rwc[:, None], dnc[:, None]], 1).astype(np.float32)
        rs = np.concatenate([obs_, rws[:, None], dns[:, None]], 1).astype(np.float32)
        same = (sc.view(np.uint32) == ss.view(np.uint32)).all(axis=1) & (rc.view(np.uint32) == rs.view(np.uint32)).all(axis=1)
        exact += int(same.sum())
        if not motor_closed_taken(k):
            assert same.all(), "%d sweeps: no closed form applies, yet envs %r differ from the sequential rows in step %d" % (k, np.nonzero(~same)[0].tolist(), t)
        assert np.array_equal(dnc, dns)
        parity.merge_worst(worst, parity.panda_quantities(sc, ss.astype(np.float64), obc, rs.astype(np.float64), rwc))
    rep = {"iters": k, "worst": worst, "bitwise_equal_env_steps": exact, "env_steps": n * steps}
    if motor_closed_taken(k):
        parity.assert_within(worst, dict((kk, (0.5 if kk in ("obj_w", "obj_v") else 0.25) * v) for kk, v in parity.TOL.items()),
                             "(%d sweeps: closed forms against the sequential rows)" % k)
        assert exact < n * steps, "%d sweeps: every env-step is bit-identical to the sequential rows -- the closed form was not taken" % k
    return rep


# ---------------------------------------------------------------------------------------------- A2
class ActionSequence:
    """stands in for the rng of parity.check_single_steps: recorded actions, one batch per step"""

    def __init__(self, acts):
        self.acts, self.k = [np.asarray(a, np.float32) for a in acts], 0

    def uniform(self, lo, hi, shape):
        a = self.acts[self.k]
        self.k += 1
        assert tuple(shape) == a.shape
        return a.copy()


def free_pair(Engine, lib, table, n):
    eng, ora = parity.make_pair(Engine, lib, table, n)
    st = parity.check_reset(eng, ora, n)            # at the default count, the usual bounds
    ora32 = orc.Oracle(table, f32=True, task=1)
    ora32.task.obj_pose_rnd_std, ora32.task.tg_pose_rnd_std = ora.task.obj_pose_rnd_std, ora.task.tg_pose_rnd_std
    return eng, ora, ora32, st


def check_free_steps(eng, ora, ora32, st, k, steps=3, seed=0, label=""):
    """Free-space steps after a default-count reset against the fp64 oracle at k sweeps: parity.check_single_steps, nothing skipped, TOL as it
    stands -- except for obj_w below OC_MIN sweeps, where the object block runs a handful of explicit sweeps over a resting cube and the
    solve has not yet contracted the rounding of its input: there the bound is max(TOL["obj_w"], 4 x d32), d32 being the deviation of the
    oracle's OWN fp32 build from the fp64 oracle in obj_w over the same states, actions and count (the rule, and the margin, that
    tests/test_gpu_kin_query.py uses for states outside its tolerance's measured range).  Prints d32 and the engine's figure."""
    n = len(st)
    parity.set_solver_iters(eng, k, ora, ora32)
    try:
        rng = np.random.default_rng(seed)
        acts, d32, s = [], 0.0, np.asarray(st, np.float64)
        for _ in range(steps):
            a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
            s32 = s.astype(np.float32)
            s, _ = ora.batch_step(s32.astype(np.float64), a)
            s_f, _ = ora32.batch_step(s32, a)
            d32 = max(d32, float(np.abs(np.asarray(s_f, np.float64)[:, 28:31] - s[:, 28:31]).max()))
            acts.append(a)
        tol = dict(parity.TOL)
        if k < OC_MIN:
            tol["obj_w"] = max(parity.TOL["obj_w"], 4.0 * d32)
        rep = {}
        try:
            parity.check_single_steps(eng, ora, st, ActionSequence(acts), steps=steps, tol=tol, report=rep)
        finally:
            fig = {"iters": k, "envs": n, "steps": steps, "obj_w_d32": float("%.3g" % d32), "obj_w_bound": float("%.3g" % tol["obj_w"]),
                   "obj_w_engine": float("%.3g" % rep.get("worst", {}).get("obj_w", float("nan")))}
            print("SWEEP_COUNTS " + json.dumps(dict(fig, engine=label)))
        assert rep["skipped_ambiguous"] == 0 and rep["compared"] == n * steps
        return fig
    finally:
        parity.set_solver_iters(eng, 150, ora, ora32)


def contact_pair(Engine, lib, panda, flags, n_each=12):
    _, ora = parity.make_pair(Engine, lib, panda["table"], 1)
    base, _ = ora.batch_reset(1)
    S = parity.contact_states(ora, panda, base[0], np.random.default_rng(1), n_each, n_each)
    eng, ora = parity.make_pair(Engine, lib, panda["table"], len(S), flags=flags)
    eng.reset()
    ora32 = orc.Oracle(panda["table"], f32=True, task=1)
    ora32.task.obj_pose_rnd_std, ora32.task.tg_pose_rnd_std = ora.task.obj_pose_rnd_std, ora.task.tg_pose_rnd_std
    return eng, (ora, ora32), S


def check_contact_steps(eng, oras, S, k, seed=5):
    """crafted contact-rich states (robot-table and robot-object contacts), one step at k sweeps against the oracle: TOL_CONTACT.  Which
    states are compared is the oracle's verdict alone (parity.check_single_steps: a contact candidate within 3 um of the margin, or a result
    that the fp64 oracle's own rounding-level perturbations or its fp32 build move by more than half the bounds -- more sweeps amplify
    rounding further, so at 300 sweeps the probe drops one state more than at 150), bounded by max_skip and the same for every engine."""
    ora, ora32 = oras
    parity.set_solver_iters(eng, k, ora, ora32)
    try:
        return parity.check_single_steps(eng, ora, S, np.random.default_rng(seed), steps=1, tol=parity.TOL_CONTACT, skip_ambiguous=True, max_skip=0.2,
                                         ora32=ora32)
    finally:
        parity.set_solver_iters(eng, 150, ora, ora32)


# ---------------------------------------------------------------------------------------------- A3
@functools.lru_cache(maxsize=None)
def _family_at(panda_key, kind, k):
    panda = row_paths._PANDA[panda_key]
    it = (("solver_iters", k),)
    if kind == "ro":
        return row_paths.family_ro(panda, it, "ro", row_paths.SEED + 1)
    if kind == "zip":
        return row_paths.family_zip(panda, it, "zip", row_paths.SEED + 2)
    if kind == "ro_clamp":
        return row_paths.family_ro(panda, row_paths.CLAMP + it, "ro_clamp", row_paths.SEED + 4)
    if kind == "clamp":
        return row_paths.family_zip(panda, row_paths.CLAMP + it, "clamp", row_paths.SEED + 3, keep=((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 1, 0), (0, 0, 1, 1)))
    raise KeyError(kind)


def family_at(panda, kind, k):
    """the family `kind` of tests/row_paths.py with solver_iters = k in its oracles (pre-filter included) and its engines; cached"""
    row_paths._PANDA[id(panda)] = panda
    fam = _family_at(id(panda), kind, k)
    assert int(fam.lab.ora.params.solver_iters) == k and int(fam.lab.ora32.params.solver_iters) == k
    return fam


def family_engine(fam, lib, k):
    eng = fam.lab.engine(_capi.Engine, lib, fam.n, fam.flags)
    assert eng.get_physics().solver_iters == k
    return eng


# ---------------------------------------------------------------------------------------------- A4
def check_residual_exit_at(Engine, lib, table, k, n=32, steps=2, **kw):
    """parity.check_residual_threshold (threshold 1e-7) with engine and oracle switched to k sweeps after the default reset; whether any env
    must leave the loop early is taken from the oracle's own sweep counts (expect_early=None)"""
    rep = parity.check_residual_threshold(Engine, lib, table, n=n, steps=steps, solver_iters=k, expect_early=None, **kw)
    return rep


def check_residual_exit_wave_mates_and_sharding(Engine, lib, panda, k, n=1024, steps=16):
    """test_solver_residual_threshold_results_do_not_depend_on_wave_mates_or_sharding at k sweeps: two engines side by side and a 2-shard
    split of the same batch, bit-identical rows, states and sweep counts.  The actions' sizes differ from env to env by three orders of
    magnitude, so the lanes of a wave leave the loop at different sweeps (the per-lane exponents of obj_closed<PERLANE>, motor_scan's exit
    pair)."""
    kw = dict(task=1, obj_pose_rnd_std=0.05, tg_pose_rnd_std=0.2, lib=lib, flags=_capi.F_AUTO_RESET, max_steps=12)
    a = Engine(panda["table"], num_envs=n, **kw)
    b = Engine(panda["table"], num_envs=n, **kw)
    h0 = Engine(panda["table"], num_envs=n // 2, env_id_base=0, **kw)
    h1 = Engine(panda["table"], num_envs=n // 2, env_id_base=n // 2, **kw)
    _, ora = parity.make_pair(Engine, lib, panda["table"], 1)
    base, _ = ora.batch_reset(1)
    S = parity.contact_states(ora, panda, base[0], np.random.default_rng(1), 8, 8).astype(np.float32)
    for e in (a, b, h0, h1):
        e.reset()
        parity.set_solver_iters(e, k)
        e.set_physics(solver_residual_threshold=1e-7)
    st = a.get_state()
    st[:len(S), :S.shape[1]] = S
    a.set_state(st); b.set_state(st); h0.set_state(st[:n // 2]); h1.set_state(st[n // 2:])
    rng = np.random.default_rng(12)
    exits = set()
    for _ in range(steps):
        act = (rng.uniform(-1, 1, (n, 7)) * 10.0 ** rng.uniform(-3, 0, (n, 1))).astype(np.float32)
        ra, rb, r0, r1 = a.step(act), b.step(act), h0.step(act[:n // 2]), h1.step(act[n // 2:])
        for x, y, z0, z1 in zip(ra, rb, r0, r1):
            assert np.array_equal(x, y) and np.array_equal(x, np.concatenate([z0, z1]))
        sw = a.get_sweeps()
        assert np.array_equal(sw, b.get_sweeps()) and np.array_equal(sw, np.concatenate([h0.get_sweeps(), h1.get_sweeps()]))
        assert sw.min() >= 1 and sw.max() <= k
        exits |= set(int(x) for x in sw)
    assert np.array_equal(a.get_state(), b.get_state())
    for e in (a, b, h0, h1):
        e.close()
    return sorted(exits)


# ---------------------------------------------------------------------------------------------- A5
def icub_group(Engine, lib, task, n):
    """iCub, joint control: engine and oracle reset at the default count, then three default-count oracle steps"""
    eng, ora, info = parity.make_icub_pair(Engine, lib, n, task, "l", 0, 0, 1, obj_std=0.05, tg_std=0.2)
    eng.reset()
    st, _ = ora.batch_reset(n)
    rng = np.random.default_rng(31)
    for _ in range(3):
        st, _ = ora.batch_step(st.astype(np.float32).astype(np.float64), rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32))
    return eng, ora, st


def check_icub_steps(eng, ora, st, k, steps=3, seed=33):
    """single steps at k sweeps from identical fp32 states against the oracle: TOL_ICUB as it stands"""
    n = len(st)
    parity.set_solver_iters(eng, k, ora)
    try:
        rng = np.random.default_rng(seed)
        worst = {}
        for _ in range(steps):
            a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
            s32 = st.astype(np.float32)
            eng.set_state(s32)
            ob, rw, dn = eng.step(a)
            st, out = ora.batch_step(s32.astype(np.float64), a)
            parity.merge_worst(worst, parity.group_quantities(eng, eng.get_state(), st, ob, out))
            assert (dn == out[:, -1]).all()
        parity.assert_within(worst, parity.TOL_ICUB, "(iCub, joint control, %d sweeps, %d envs x %d steps)" % (k, n, steps))
        return worst
    finally:
        parity.set_solver_iters(eng, 150, ora)


def hands_group(Engine, lib, n):
    """iCub with hands, right arm, joint control, the controlled hand's finger motors set as in parity.check_hands: default-count reset, then
    two default-count oracle steps"""
    from pybullet_robot_envs.model.table import GRASP_POS
    eng, ora, info = parity.make_hands_pair(Engine, lib, n, "r", 0)
    eng.reset()
    st, mrec, _ = ora.hands_reset(n)
    pos = list(GRASP_POS)
    eng.set_motors(info["fingers"], pos, 0.1, 10.0)
    mrec = ora.hands_set_motors(mrec, info["fingers"], pos, 0.1, 10.0)
    home = np.asarray(info["home"])[info["controlled"]]
    rng = np.random.default_rng(35)
    for _ in range(2):
        a = (home[None, :] + rng.uniform(-0.2, 0.2, (n, len(home)))).astype(np.float32)
        st, mrec, _ = ora.hands_step(st.astype(np.float32).astype(np.float64), mrec, a)
    return eng, ora, st, mrec, home


def check_hands_steps(eng, ora, st, mrec, home, k, steps=2, seed=37):
    n = len(st)
    parity.set_solver_iters(eng, k, ora)
    try:
        rng = np.random.default_rng(seed)
        worst = {}
        for _ in range(steps):
            a = (home[None, :] + rng.uniform(-0.2, 0.2, (n, len(home)))).astype(np.float32)
            s32 = st.astype(np.float32)
            eng.set_state(s32)
            ob, rw, dn = eng.step(a)
            st, mrec, out = ora.hands_step(s32.astype(np.float64), mrec, a)
            parity.merge_worst(worst, parity.group_quantities(eng, eng.get_state(), st, ob, out, tail=7))
            assert (dn == out[:, -1]).all()
        parity.assert_within(worst, parity.TOL_HANDS, "(iCub with hands, %d sweeps, %d envs x %d steps)" % (k, n, steps))
        return worst
    finally:
        parity.set_solver_iters(eng, 150, ora)


def odd_exit_figures(eng, k, step_engine, step_oracle, set_oracle_iters):
    """joint velocities after one step at k sweeps: per env, the engine's distance from the oracle at k sweeps (err) and the oracle's own
    distance between k and k + 1 sweeps (gap)"""
    nd, vo = eng.ndof, eng.v_off
    parity.set_solver_iters(eng, k)
    try:
        se = np.asarray(step_engine(), np.float64)[:, vo:vo + nd]
        set_oracle_iters(k)
        so_k = step_oracle()[:, vo:vo + nd]
        set_oracle_iters(k + 1)
        so_k1 = step_oracle()[:, vo:vo + nd]
    finally:
        parity.set_solver_iters(eng, 150)
        set_oracle_iters(150)
    return np.abs(se - so_k).max(axis=1), np.abs(so_k1 - so_k).max(axis=1)


def assert_odd_exit(err, gap, k, what):
    """At 1 and 3 sweeps a solve under random commands is far from converged: one sweep more moves the joint velocities by orders of
    magnitude more than fp32 rounding does.  So an engine whose two-sweeps-per-trip loop misses its odd-count exit -- and runs k + 1 sweeps --
    is told from a correct one without any tolerance on the engine's error: it lands ON the oracle's (k + 1)-sweep result, a correct one
    within a tenth of the way there.  (The tolerance-based comparisons cannot run at these counts for the lane-group engines: there the
    oracle's own fp32 build misses the bounds)"""
    print("ODD_EXIT %s, %d sweeps: engine - oracle(k) %r, oracle(k + 1) - oracle(k) %r" % (what, k, [float("%.3g" % x) for x in err], [float("%.3g" % x) for x in gap]))
    assert (gap > 0).all() and (err < 0.1 * gap).all(), "%s at %d sweeps: the result is not the %d-sweep one (err %r, gap to %d sweeps %r)" % (what, k, k, err, k + 1, gap)


def check_icub_odd_exit(eng, ora, st, k, seed=39):
    n = len(st)
    a = np.random.default_rng(seed).uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
    s32 = st.astype(np.float32)

    def step_engine():
        eng.set_state(s32)
        eng.step(a)
        return eng.get_state()
    err, gap = odd_exit_figures(eng, k, step_engine, lambda: ora.batch_step(s32.astype(np.float64), a)[0], lambda i: setattr(ora.params, "solver_iters", i))
    assert_odd_exit(err, gap, k, "iCub")


def check_hands_odd_exit(eng, ora, st, mrec, home, k, seed=41):
    n = len(st)
    a = (home[None, :] + np.random.default_rng(seed).uniform(-0.2, 0.2, (n, len(home)))).astype(np.float32)
    s32 = st.astype(np.float32)

    def step_engine():
        eng.set_state(s32)
        eng.step(a)
        return eng.get_state()
    err, gap = odd_exit_figures(eng, k, step_engine, lambda: ora.hands_step(s32.astype(np.float64), mrec, a)[0], lambda i: setattr(ora.params, "solver_iters", i))
    assert_odd_exit(err, gap, k, "iCub with hands")
