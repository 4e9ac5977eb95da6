"""Reference of the batched inverse-kinematics query (include/pbre_ik.h; csrc/pbre_ik.hip): damped least squares on the chain from the
root to one link, in numpy, vectorised over the envs, written from the definition (oracle/pbre_oracle.c: orc_ik is its float64 anchor,
test_ik_host.py):

  from q = q_start, at most max_iters times:
    x, R   the point's world position and the link's rotation at q           (contact_ref.link_frames: the whole tree)
    e      = [target_pos - x ; rotvec(R_target R^T)]                         (position rows alone without target_quat)
    stop   when |e_pos| < residual (and, with rot_residual > 0, angle < rot_residual) -- before the update
    q     += J^T (J J^T + damping^2 I)^-1 e                                  (Cholesky; kin_ref.point_jacobian, columns of DoFs that move)

A DoF moves if it is on the chain, its link is not ik_passive and its dof_mask byte (if any) is non-zero.  `dtype` selects the arithmetic
of everything: np.float64 is the reference, np.float32 the same formulas in single precision (the GPU tolerances' yardstick)."""
import numpy as np

from pybullet_robot_envs.model.table import HEADER, LINK_STRIDE

import contact_ref
import kin_ref


def chain_info(table, link=None, dof_mask=None):
    """K (kin_ref.links_of) plus: the driven link, `moving` [nd] bool, `lower` / `upper` [nd]"""
    t = np.asarray(table, float)
    K = kin_ref.links_of(t)
    nl, nd = K["nl"], K["nd"]
    L = t[HEADER: HEADER + nl * LINK_STRIDE].reshape(nl, LINK_STRIDE)
    link = K["ee"] if link is None or link < 0 else int(link)
    moving = np.zeros(nd, bool)
    lower, upper = np.zeros(nd), np.zeros(nd)
    for i in range(nl):
        if K["jtype"][i] != 0:
            lower[K["dof"][i]], upper[K["dof"][i]] = L[i, 30], L[i, 31]
    for i in kin_ref.ancestors(K, link):
        d = K["dof"][i]
        if K["jtype"][i] != 0 and L[i, 37] == 0 and (dof_mask is None or dof_mask[d]):
            moving[d] = True
    return K, link, moving, lower, upper


def quat_to_R(quat, dt):
    q = np.asarray(quat, dt)
    q = q / np.sqrt((q * q).sum(axis=-1, keepdims=True))
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    one, two = dt(1), dt(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w),
                  two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w),
                  two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)], -1)
    return R.reshape(q.shape[:-1] + (3, 3)).astype(dt)


def rotvec(E, dt):
    """world-frame rotation vector of the rotations E [N, 3, 3] and its angle, by orc_ik's formulas (the s2 > 1e-9 branch)"""
    s = np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], -1)
    s2 = np.sqrt((s * s).sum(axis=1)) * dt(0.5)
    c2 = (E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - dt(1)) * dt(0.5)
    ang = np.arctan2(s2, c2).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(s2 > dt(1e-9), ang / (dt(2) * s2), dt(0.5)).astype(dt)
    return f[:, None] * s, ang


def pose_error(table, K, link, q, point, target_pos, Rt, dt):
    """e [N, 3 or 6], |e_pos| [N], angle [N] (zeros without Rt), and R, p, x for the Jacobian"""
    R, p = contact_ref.link_frames(table, q, dt)
    x = p[:, link] + np.einsum("nij,j->ni", R[:, link], point)
    e = target_pos - x
    perr = np.sqrt((e * e).sum(axis=1))
    ang = np.zeros(len(q), dt)
    if Rt is not None:
        rv, ang = rotvec(np.einsum("nij,nkj->nik", Rt, R[:, link]), dt)
        e = np.concatenate([e, rv], axis=1)
    return e.astype(dt), perr.astype(dt), ang, R, p, x


def dls_step(J, e, l2, dt):
    """dq [N, nd] = J^T (J J^T + l2 I)^-1 e by an explicit Cholesky factorisation, every operation in dt"""
    n, m, _ = J.shape
    A = np.einsum("nad,nbd->nab", J, J).astype(dt) + l2 * np.eye(m, dtype=dt)
    L = np.zeros((n, m, m), dt)
    for a in range(m):
        for b in range(a + 1):
            s = A[:, a, b] - (L[:, a, :b] * L[:, b, :b]).sum(axis=1)
            L[:, a, b] = np.sqrt(s) if a == b else s / L[:, b, b]
    y = np.zeros((n, m), dt)
    for a in range(m):
        y[:, a] = (e[:, a] - (L[:, a, :a] * y[:, :a]).sum(axis=1)) / L[:, a, a]
    for a in range(m - 1, -1, -1):
        y[:, a] = (y[:, a] - (L[:, a + 1:, a] * y[:, a + 1:]).sum(axis=1)) / L[:, a, a]
    return np.einsum("nad,na->nd", J, y).astype(dt)


def solve(table, q_start, target_pos, target_quat=None, link=None, point=(0, 0, 0), dof_mask=None, damping=0.1, residual=1e-3,
          rot_residual=0.0, max_iters=100, clamp_limits=False, dtype=np.float64):
    """The outputs of pbre_ik_query for start values q_start [N, nd]: "q" [N, nd], "err" [N, 2], "iters" [N] int32, and the history the
    ambiguity rule needs: "hist_pos", "hist_rot" [max_iters + 1, N] -- the errors every convergence test saw (NaN: the env had stopped)."""
    dt = np.dtype(dtype).type
    table = np.asarray(table, float)
    K, link, moving, lower, upper = chain_info(table, link, dof_mask)
    q = np.array(q_start, dt)
    n = len(q)
    tp = np.asarray(target_pos, dt)
    Rt = None if target_quat is None else quat_to_R(target_quat, dt)
    pt = np.asarray(point, np.float32).astype(dt)
    l2 = dt(float(damping) * float(damping))
    res, rres = dt(np.float32(residual)), dt(np.float32(rot_residual))
    lo, hi = lower.astype(np.float32).astype(dt), upper.astype(np.float32).astype(dt)
    active = np.ones(n, bool)
    iters = np.zeros(n, np.int32)
    err = np.zeros((n, 2), dt)
    hist_pos = np.full((max_iters + 1, n), np.nan); hist_rot = np.full((max_iters + 1, n), np.nan)
    for k in range(max_iters + 1):
        e, perr, ang, R, p, x = pose_error(table, K, link, q, pt, tp, Rt, dt)
        hist_pos[k, active] = perr[active]; hist_rot[k, active] = ang[active]
        conv = perr < res
        if rres > 0:
            conv &= ang < rres
        stop = active & (conv | (iters >= max_iters))
        err[stop, 0] = perr[stop]; err[stop, 1] = ang[stop]
        active &= ~stop
        if not active.any():
            break
        J = kin_ref.point_jacobian(K, R, p, link, x, dt)[:, :e.shape[1]]
        J[:, :, ~moving] = 0
        qn = q + dls_step(J, e, l2, dt)
        if clamp_limits:
            qn[:, moving] = np.minimum(np.maximum(qn[:, moving], lo[moving]), hi[moving])
        q[active] = qn[active]
        iters[active] += 1
    assert q.dtype == dt and err.dtype == dt
    return dict(q=q, err=err, iters=iters, hist_pos=hist_pos, hist_rot=hist_rot)


def ambiguous(r, tol_pos, residual=1e-3, tol_rot=0.0, rot_residual=0.0):
    """[N] bool: at some convergence test the reference's position error lay within tol_pos of `residual` (with rot_residual > 0: or its
    rotation error within tol_rot of rot_residual) -- float32 arithmetic may legitimately decide that test the other way.  With
    residual = 0 no error, in any arithmetic, is below it: there is no decision and no env is ambiguous."""
    with np.errstate(invalid="ignore"):
        amb = (np.abs(r["hist_pos"] - residual) <= tol_pos).any(axis=0) & (residual > 0)
        if rot_residual > 0:
            amb |= (np.abs(r["hist_rot"] - rot_residual) <= tol_rot).any(axis=0)
    return amb
