"""Reference of the batched contact query (include/pbre_contacts.h; csrc/pbre_contacts.hip): all five outputs for a batch of state
records, in numpy.  The pair set and the detection rule are model/contacts.py: contact_flags (which test_contact_host.py holds this
module to); the distances come from that module's own helpers -- _sphere_box_dist, _sphere_round_dist, _closest_on_triangles, _quat_R,
_shape_candidates -- and the link frames from the formulas of its link_frames.

`dtype` selects the arithmetic of everything, the forward kinematics included: np.float64 is the reference, np.float32 the same formulas
in single precision -- what test_contact_host.py measures REF32_DIST with.  Hull distances are exact here (no bounding-sphere early-out)."""
import numpy as np

from pybullet_robot_envs.model import contacts as mc
from pybullet_robot_envs.model.objects import hull_pieces
from pybullet_robot_envs.model.table import HEADER, LINK_STRIDE, SPHERE_STRIDE

FAR = np.float32(3.0e38)          # PBRE_CQ_FAR
OBJECT_TABLE, ROBOT_OBJECT, ROBOT_TABLE = mc.OBJECT_TABLE, mc.ROBOT_OBJECT, mc.ROBOT_TABLE


def link_frames(table, q, dtype=np.float64):
    """contacts.link_frames with every array in `dtype` (float64: the same numbers, test_contact_host.py)"""
    dt = np.dtype(dtype).type
    table = np.asarray(table, float)
    nl, n = int(table[2]), q.shape[0]
    q = np.asarray(q, dt)
    T = table.astype(dt)
    Rb, pb = T[9:18].reshape(3, 3), T[6:9]
    R = np.empty((n, nl, 3, 3), dt); p = np.empty((n, nl, 3), dt)
    eye = np.eye(3, dtype=dt)
    for i in range(nl):
        r = T[HEADER + i * LINK_STRIDE: HEADER + (i + 1) * LINK_STRIDE]
        ri = table[HEADER + i * LINK_STRIDE: HEADER + (i + 1) * LINK_STRIDE]
        par, jt, axis, xyz, R0, dof = int(ri[0]), int(ri[1]), r[2:5], r[5:8], r[8:17].reshape(3, 3), int(ri[33])
        Rp = R[:, par] if par >= 0 else np.broadcast_to(Rb, (n, 3, 3))
        pp = p[:, par] if par >= 0 else np.broadcast_to(pb, (n, 3))
        if jt == 1:
            a = axis
            K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dt)
            s, c = np.sin(q[:, dof])[:, None, None], np.cos(q[:, dof])[:, None, None]
            Rl = R0[None] @ (eye[None] + s * K[None] + (1 - c) * (K @ K)[None]); pl = np.broadcast_to(xyz, (n, 3))
        elif jt == 2:
            Rl = np.broadcast_to(R0, (n, 3, 3)); pl = xyz[None] + (R0 @ axis)[None] * q[:, dof, None]
        else:
            Rl = np.broadcast_to(R0, (n, 3, 3)); pl = np.broadcast_to(xyz, (n, 3))
        R[:, i] = Rp @ Rl
        p[:, i] = pp + np.einsum("nij,nj->ni", Rp, pl)
    assert R.dtype == dt and p.dtype == dt
    return R, p


def hull_faces(hull, dtype=np.float64):
    """per piece of an `obj_hull` vertex list: (vertices [nv, 3], plane normals [nf, 3], plane offsets [nf], triangles [nt, 3, 3])"""
    from scipy.spatial import ConvexHull
    out = []
    for pc in hull_pieces(hull):
        H = ConvexHull(pc)
        out.append((pc.astype(dtype), H.equations[:, :3].astype(dtype), H.equations[:, 3].astype(dtype), pc[H.simplices].astype(dtype)))
    return out


def _piece_dist(dl, sr, piece):
    """contacts._sphere_hull_dist behind the object frame, in the dtype of its arguments"""
    _, nrm, off, tri = piece
    sd = (dl @ nrm.T + off[None]).max(axis=1)
    dist = np.sqrt(mc._closest_on_triangles(dl, tri[:, 0], tri[:, 1], tri[:, 2]).min(axis=1)).astype(dl.dtype)
    return np.where(sd <= 0, sd - sr, dist - sr)


def sphere_centres(table, state, dtype=np.float64):
    """world centres [N, ns, 3] and radii [ns] of the RobotTable's collision spheres, fingertip slots + 1 [ns], links [ns]"""
    dt = np.dtype(dtype).type
    table = np.asarray(table, float)
    nl, ns = int(table[2]), int(table[5])
    st = np.asarray(state)
    R, p = link_frames(table, st[:, :int(table[3])], dt)
    sph = table[HEADER + nl * LINK_STRIDE: HEADER + nl * LINK_STRIDE + ns * SPHERE_STRIDE].reshape(ns, SPHERE_STRIDE)
    sc = np.empty((st.shape[0], ns, 3), dt)
    for k in range(ns):
        li = int(sph[k, 0])
        sc[:, k] = p[:, li] + np.einsum("nij,j->ni", R[:, li], sph[k, 1:4].astype(dt))
    return sc, sph[:, 4].astype(dt), sph[:, 6].astype(int), sph[:, 0].astype(int)


def sphere_object_dist(c, r, op, Ro, shape, oh, pieces):
    """signed distance of the spheres (centres c[N, 3], radius r) to the objects at op[N, 3] with rotations Ro[N, 3, 3]; pieces: hull_faces()"""
    if shape == 3:
        dl = np.einsum("nji,nj->ni", Ro, c - op)
        return np.min([_piece_dist(dl, r, pc) for pc in pieces], axis=0)
    if shape == 0:
        return mc._sphere_box_dist(c, r, op, Ro, oh)
    return mc._sphere_round_dist(shape, c, r, op, Ro, oh)


def query(table, state, obj_off, phys, margin=None, no_object=False, hull=None, dtype=np.float64):
    """The five outputs of pbre_contact_query for the records state[N, F] -- "flags" int32 [N], "dist" [N, 3] (dtype), "nearest" int32
    [N, 2], "count" int32 [N, 2], "tips" int32 [N] -- and what they were reduced from: "d_ro", "d_rt" [N, ns] per-sphere distances to the
    object / the table (d_ro: FAR without an object), "d_ot" [N, nc] per-candidate z - top (FAR where the candidate does not count) and
    "edge" [N]: how close (m) any candidate comes to the boundary of "over the table top, above its underside".
    margin None or negative: phys.contact_margin."""
    dt = np.dtype(dtype).type
    st = np.asarray(state)
    n = st.shape[0]
    sc, sr, slot, _ = sphere_centres(table, st, dt)
    ns = len(sr)
    mg = dt(phys.contact_margin) if margin is None or margin < 0 else dt(np.float32(margin))
    tc, th = np.array(list(phys.table_c), dt), np.array(list(phys.table_h), dt)
    oh = np.array(list(phys.obj_h), dt)
    shape = int(getattr(phys, "obj_shape", 0))
    op, Ro = st[:, obj_off:obj_off + 3].astype(dt), mc._quat_R(st[:, obj_off + 3:obj_off + 7].astype(dt)).astype(dt)
    eye = np.broadcast_to(np.eye(3, dtype=dt), (n, 3, 3))
    far = dt(FAR)
    d_ro, d_rt = np.full((n, ns), far, dt), np.full((n, ns), far, dt)
    pieces = hull_faces(hull, dt) if (shape == 3 and not no_object) else None
    for k in range(ns):
        c, r = sc[:, k], sr[k]
        d_rt[:, k] = mc._sphere_box_dist(c, r, np.broadcast_to(tc, (n, 3)), eye, th)
        if no_object:
            continue
        d_ro[:, k] = sphere_object_dist(c, r, op, Ro, shape, oh, pieces)
    if no_object:
        d_ot, edge = np.full((n, 1), far, dt), np.full(n, np.inf)
    else:
        top, bot = tc[2] + th[2], tc[2] - th[2]
        if shape == 3:
            hv = np.concatenate([pc[0] for pc in pieces])
            cand = np.einsum("nij,vj->nvi", Ro, hv); ok = np.ones(cand.shape[:2], bool)
        else:
            cand, ok = mc._shape_candidates(shape, oh, Ro)
            cand = cand.astype(dt)
        x = op[:, None, :] + cand
        gaps = np.stack([np.abs(np.abs(x[..., 0] - tc[0]) - th[0]), np.abs(np.abs(x[..., 1] - tc[1]) - th[1]), np.abs(x[..., 2] - bot)], -1).min(-1)
        edge = np.where(ok, gaps, np.inf).min(axis=1)
        on = (np.abs(x[..., 0] - tc[0]) <= th[0]) & (np.abs(x[..., 1] - tc[1]) <= th[1]) & (x[..., 2] > bot) & ok
        d_ot = np.where(on, x[..., 2] - top, far).astype(dt)
    res = {"d_ro": d_ro, "d_rt": d_rt, "d_ot": d_ot, "edge": edge, "margin": mg}
    dist = np.full((n, 3), far, dt)
    nearest = np.full((n, 2), -1, np.int32)
    count = np.zeros((n, 2), np.int32)
    tips = np.zeros(n, np.int32)
    dist[:, 0] = d_ot.min(axis=1)
    if ns:
        dist[:, 2] = d_rt.min(axis=1); nearest[:, 1] = d_rt.argmin(axis=1); count[:, 1] = (d_rt < mg).sum(axis=1)
        if not no_object:
            dist[:, 1] = d_ro.min(axis=1); nearest[:, 0] = d_ro.argmin(axis=1); count[:, 0] = (d_ro < mg).sum(axis=1)
            for k in range(ns):
                if slot[k] > 0:
                    tips |= np.where(d_ro[:, k] < mg, 1 << (slot[k] - 1), 0).astype(np.int32)
    flags = (np.where(dist[:, 0] < mg, OBJECT_TABLE, 0) | np.where(count[:, 0] > 0, ROBOT_OBJECT, 0) | np.where(count[:, 1] > 0, ROBOT_TABLE, 0)).astype(np.int32)
    assert dist.dtype == dt
    res.update(flags=flags, dist=dist, nearest=nearest, count=count, tips=tips)
    return res


def band(ref, tol):
    """[N] bool: some pair's reference distance is within tol of the margin (flags, count and tips may legitimately differ there)"""
    mg = float(ref["margin"])
    near = lambda d: (np.abs(d.astype(float) - mg) <= tol).any(axis=1)
    return near(ref["d_ro"]) | near(ref["d_rt"]) | near(ref["d_ot"])


def ambiguous_nearest(ref, tol):
    """[N, 2] bool: the two smallest per-sphere distances differ by less than tol (either index is right)"""
    out = np.zeros((ref["d_ro"].shape[0], 2), bool)
    for j, d in enumerate((ref["d_ro"], ref["d_rt"])):
        if d.shape[1] >= 2:
            s = np.sort(d.astype(float), axis=1)
            out[:, j] = ((s[:, 1] - s[:, 0]) < tol) & (s[:, 0] < 1e38)       # (no object: every entry is FAR and `nearest` is -1)
    return out


def compare(ref, got, tol, what="", hull_reach=None):
    """The GPU tests' comparison rule: `dist` within tol; flags, count and tips equal outside band(ref, tol); nearest equal unless
    ambiguous within 2 tol.  hull_reach (margin + the largest piece radius) for a hull object: dist[1] and nearest[0] are compared only
    where the reference is below it (above, the query may return a lower bound that is >= margin instead).  Returns the left-out mask [N]."""
    d_ref, d_got = ref["dist"].astype(float), np.asarray(got["dist"], float)
    far = d_ref > 1e38
    assert np.array_equal(far, d_got > 1e38), "%s: PBRE_CQ_FAR entries differ" % what
    cmp1 = np.ones(len(d_ref), bool) if hull_reach is None else d_ref[:, 1] < hull_reach - 1e-5     # (the device's reach is a rounded float)
    err = np.where(far, 0.0, np.abs(d_ref - d_got))
    if hull_reach is not None:
        lower = ~cmp1 & ~far[:, 1] & (err[:, 1] > tol)
        assert (d_got[lower, 1] <= d_ref[lower, 1] + tol).all() and (d_got[lower, 1] >= float(ref["margin"])).all(), "%s: not a lower bound >= margin" % what
        err[~cmp1, 1] = 0.0
    print("%s: %d envs, largest |dist - ref| %.3g (allowed %.3g)" % (what, len(d_ref), err.max() if err.size else 0.0, tol))
    assert (err <= tol).all(), "%s: dist off by %g" % (what, err.max())
    out = band(ref, tol)
    keep = ~out
    for k in ("flags", "count", "tips"):
        assert np.array_equal(np.asarray(got[k])[keep], ref[k][keep]), "%s: %s differ outside the band" % (what, k)
    amb = ambiguous_nearest(ref, 2 * tol)
    g = np.asarray(got["nearest"])
    for j in range(2):
        chk = ~amb[:, j] & (cmp1 if j == 0 else True)
        assert np.array_equal(g[chk, j], ref["nearest"][chk, j]), "%s: nearest[%d] differs" % (what, j)
        # an ambiguous one still names a sphere that is within 2 tol of the smallest
        d = ref["d_ro"] if j == 0 else ref["d_rt"]
        for e in np.flatnonzero(amb[:, j] & (cmp1 if j == 0 else True)):
            assert g[e, j] >= 0 and d[e, g[e, j]] - d[e].min() < 2 * tol, "%s: nearest[%d] of env %d" % (what, j, e)
    return out
