"""Reference of the batched kinematics / dynamics query (include/pbre_kin.h; csrc/pbre_kin.hip): all five outputs for a batch of joint
positions, velocities and accelerations, in numpy, by the direct O(n^2) formulas -- per-link Jacobians at the centres of mass,
M = sum m Jv^T Jv + Jw^T Ic Jw, tau = sum Jv^T f + Jw^T n -- which share nothing with the device's recursions (composite bodies, RNEA) nor
with the oracle (articulated bodies).  test_kin_host.py holds this module to the oracle in float64.

`dtype` selects the arithmetic of everything: np.float64 is the reference, np.float32 the same formulas in single precision -- what
test_kin_host.py measures the GPU tolerances with.

World-frame recursions (link i, parent p, a_i = R_i axis_i, r = p_i - p_p, base at rest accelerated by (0, 0, -gravity_z)):
  revolute   w_i = w_p + a_i qd, v_i = v_p + w_p x r, al_i = al_p + a_i qdd + (w_p x a_i) qd, acc_i = acc_p + al_p x r + w_p x (w_p x r)
  prismatic  w, al as the parent's; v_i = ... + a_i qd; acc_i = ... + a_i qdd + 2 (w_p x a_i) qd"""
import numpy as np

from pybullet_robot_envs.model.table import HEADER, LINK_STRIDE

import contact_ref


def links_of(table):
    """per link of a RobotTable: parent, joint type, DoF index (int arrays), axis, mass, com, inertia (float64)"""
    t = np.asarray(table, float)
    nl = int(t[2])
    L = t[HEADER: HEADER + nl * LINK_STRIDE].reshape(nl, LINK_STRIDE)
    return dict(nl=nl, nd=int(t[3]), ee=int(t[4]), parent=L[:, 0].astype(int), jtype=L[:, 1].astype(int), dof=L[:, 33].astype(int),
                axis=L[:, 2:5], mass=L[:, 17], com=L[:, 18:21], inertia=L[:, 21:30].reshape(nl, 3, 3), damping=L[:, 32], xyz=L[:, 5:8],
                R0=L[:, 8:17].reshape(nl, 3, 3))


def ancestors(K, i):
    """link i and its ancestors, from i to the root"""
    out = []
    while i >= 0:
        out.append(i)
        i = int(K["parent"][i])
    return out


def quat_of(R):
    """[..., 3, 3] rotations -> [..., 4] quaternions x, y, z, w with w >= 0: the branch on the largest of the trace and the diagonal terms"""
    R = np.asarray(R)
    dt = R.dtype.type
    flat = R.reshape(-1, 3, 3)
    out = np.empty((len(flat), 4), R.dtype)
    one, two, quarter = dt(1), dt(2), dt(0.25)
    for n, M in enumerate(flat):
        tr = M[0, 0] + M[1, 1] + M[2, 2]
        if tr >= M[0, 0] and tr >= M[1, 1] and tr >= M[2, 2]:
            s = two * np.sqrt(one + tr)
            q = [(M[2, 1] - M[1, 2]) / s, (M[0, 2] - M[2, 0]) / s, (M[1, 0] - M[0, 1]) / s, quarter * s]
        elif M[0, 0] >= M[1, 1] and M[0, 0] >= M[2, 2]:
            s = two * np.sqrt(one + M[0, 0] - M[1, 1] - M[2, 2])
            q = [quarter * s, (M[0, 1] + M[1, 0]) / s, (M[0, 2] + M[2, 0]) / s, (M[2, 1] - M[1, 2]) / s]
        elif M[1, 1] >= M[2, 2]:
            s = two * np.sqrt(one + M[1, 1] - M[0, 0] - M[2, 2])
            q = [(M[0, 1] + M[1, 0]) / s, quarter * s, (M[1, 2] + M[2, 1]) / s, (M[0, 2] - M[2, 0]) / s]
        else:
            s = two * np.sqrt(one + M[2, 2] - M[0, 0] - M[1, 1])
            q = [(M[0, 2] + M[2, 0]) / s, (M[1, 2] + M[2, 1]) / s, quarter * s, (M[1, 0] - M[0, 1]) / s]
        q = np.array(q, R.dtype)
        out[n] = -q if q[3] < 0 else q
    return out.reshape(R.shape[:-2] + (4,))


def point_jacobian(K, R, p, link, x, dtype):
    """[N, 6, nd] Jacobian (linear rows, then angular) of the world points x [N, 3] moving with `link`; R, p: contact_ref.link_frames"""
    n = R.shape[0]
    J = np.zeros((n, 6, K["nd"]), dtype)
    for j in ancestors(K, link):
        jt, d = K["jtype"][j], K["dof"][j]
        if jt == 0:
            continue
        a = np.einsum("nij,j->ni", R[:, j], K["axis"][j].astype(dtype))
        if jt == 1:
            J[:, :3, d] = np.cross(a, x - p[:, j]); J[:, 3:, d] = a
        else:
            J[:, :3, d] = a
    return J


def motion(K, R, p, qd, qdd, g_up, dtype):
    """w, v, al, acc [N, nl, 3] of every link frame by the recursions of the module's docstring"""
    n, nl = R.shape[0], K["nl"]
    w, v, al, acc = (np.zeros((n, nl, 3), dtype) for _ in range(4))
    zero = np.zeros((n, 3), dtype)
    base_acc = np.broadcast_to(np.array([0, 0, g_up], dtype), (n, 3))
    pb = None
    for i in range(nl):
        par, jt, d = K["parent"][i], K["jtype"][i], K["dof"][i]
        if par >= 0:
            wp, vp, alp, accp, r = w[:, par], v[:, par], al[:, par], acc[:, par], p[:, i] - p[:, par]
        else:
            wp, vp, alp, accp, r = zero, zero, zero, base_acc, zero       # (the base is at rest: r multiplies zeros only)
        a = np.einsum("nij,j->ni", R[:, i], K["axis"][i].astype(dtype))
        w[:, i], al[:, i] = wp, alp
        v[:, i] = vp + np.cross(wp, r)
        acc[:, i] = accp + np.cross(alp, r) + np.cross(wp, np.cross(wp, r))
        if jt == 1:
            w[:, i] = wp + a * qd[:, d, None]
            al[:, i] = alp + a * qdd[:, d, None] + np.cross(wp, a) * qd[:, d, None]
        elif jt == 2:
            v[:, i] += a * qd[:, d, None]
            acc[:, i] += a * qdd[:, d, None] + dtype(2) * np.cross(wp, a) * qd[:, d, None]
    return w, v, al, acc


def query(table, q, qd, qdd=None, gravity_z=-9.8, links=None, at_com=False, jac_link=None, jac_point=(0, 0, 0), jac_at_com=False, dtype=np.float64):
    """The five outputs of pbre_kin_query for joint positions q, velocities qd and accelerations qdd [N, nd] (None: zeros): "pose"
    [N, n_links, 7], "vel" [N, n_links, 6], "jac" [N, 6, nd], "mass" [N, nd, nd], "tau" [N, nd], all in `dtype`; also "R", "p" (the link
    frames).  links None: every link."""
    dt = np.dtype(dtype).type
    K = links_of(table)
    nl, nd = K["nl"], K["nd"]
    q, qd = np.asarray(q, dt), np.asarray(qd, dt)
    n = q.shape[0]
    qdd = np.zeros((n, nd), dt) if qdd is None else np.asarray(qdd, dt)
    R, p = contact_ref.link_frames(table, q, dt)
    com = p + np.einsum("nlij,lj->nli", R, K["com"].astype(dt))
    w, v, al, acc = motion(K, R, p, qd, qdd, dt(-gravity_z), dt)
    links = list(range(nl)) if links is None else [int(x) for x in links]
    pose = np.empty((n, len(links), 7), dt); vel = np.empty((n, len(links), 6), dt)
    for k, li in enumerate(links):
        c = com[:, li] - p[:, li] if at_com else np.zeros((n, 3), dt)
        pose[:, k, :3] = p[:, li] + c
        pose[:, k, 3:] = quat_of(R[:, li])
        vel[:, k, :3] = v[:, li] + np.cross(w[:, li], c)
        vel[:, k, 3:] = w[:, li]
    jl = K["ee"] if jac_link is None or jac_link < 0 else int(jac_link)
    x = com[:, jl] if jac_at_com else p[:, jl] + np.einsum("nij,j->ni", R[:, jl], np.asarray(jac_point, np.float32).astype(dt))
    jac = point_jacobian(K, R, p, jl, x, dt)
    M = np.zeros((n, nd, nd), dt); tau = np.zeros((n, nd), dt)
    for i in range(nl):
        m = dt(K["mass"][i])
        Ic = np.einsum("nij,jk,nlk->nil", R[:, i], K["inertia"][i].astype(dt), R[:, i])       # R Ic R^T
        J = point_jacobian(K, R, p, i, com[:, i], dt)
        Jv, Jw = J[:, :3], J[:, 3:]
        M += m * np.einsum("nki,nkj->nij", Jv, Jv) + np.einsum("nki,nkl,nlj->nij", Jw, Ic, Jw)
        c = com[:, i] - p[:, i]
        a_c = acc[:, i] + np.cross(al[:, i], c) + np.cross(w[:, i], np.cross(w[:, i], c))
        f = m * a_c
        Iw = np.einsum("nij,nj->ni", Ic, w[:, i])
        nn = np.einsum("nij,nj->ni", Ic, al[:, i]) + np.cross(w[:, i], Iw)
        tau += np.einsum("nki,nk->ni", Jv, f) + np.einsum("nki,nk->ni", Jw, nn)
    out = dict(pose=pose, vel=vel, jac=jac, mass=M, tau=tau, R=R, p=p, com=com)
    for k in ("pose", "vel", "jac", "mass", "tau"):
        assert out[k].dtype == dt, k
    return out


def potential_energy(table, q, gravity_z=-9.8):
    """[N] sum m g z of the links' centres of mass (float64)"""
    K = links_of(table)
    R, p = contact_ref.link_frames(table, np.asarray(q, float))
    com = p + np.einsum("nlij,lj->nli", R, K["com"])
    return -gravity_z * np.einsum("l,nl->n", K["mass"], com[:, :, 2])


def errors(ref, got):
    """The six figures the tolerances are stated in, of `got` against `ref` (dicts of the five outputs): "pos" (m), "quat", "vel", "jac",
    "mass" (|dM_ij| / sqrt(M_ii M_jj)), "tau" (|dtau_j| / (1 + |tau_j|)); an output missing from `got` is left out.  Quaternions q and -q are the
    same rotation: where the reference's w is below 1e-3 the sign rule w >= 0 may legitimately pick either, and the nearer one is compared."""
    f = lambda a: np.asarray(a, float)
    out = {}
    if "pose" in got:
        out["pos"] = np.abs(f(got["pose"])[..., :3] - f(ref["pose"])[..., :3]).max(initial=0.0)
        a, b = f(got["pose"])[..., 3:], f(ref["pose"])[..., 3:]
        d = np.abs(a - b).max(axis=-1)
        d = np.where(np.abs(b[..., 3]) < 1e-3, np.minimum(d, np.abs(a + b).max(axis=-1)), d)
        out["quat"] = d.max(initial=0.0)
    for k in ("vel", "jac"):
        if k in got:
            out[k] = np.abs(f(got[k]) - f(ref[k])).max(initial=0.0)
    if "mass" in got:
        M = f(ref["mass"])
        dg = np.sqrt(np.einsum("nii->ni", M))
        out["mass"] = (np.abs(f(got["mass"]) - M) / (dg[:, :, None] * dg[:, None, :])).max(initial=0.0)
    if "tau" in got:
        t = f(ref["tau"])
        out["tau"] = (np.abs(f(got["tau"]) - t) / (1 + np.abs(t))).max(initial=0.0)
    return out
