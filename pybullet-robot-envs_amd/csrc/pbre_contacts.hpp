// pbre_contacts.hpp -- per-pair distance functions of the contact query (include/pbre_contacts.h): a robot collision sphere against the
// table box and against the object (box, sphere, cylinder, hull, compound), and the object's candidate points against the table top.
// PBRE_HD as in pbre_math.hpp: the same header compiles for the device (pbre_contacts.hip) and for the host (tests/contact_host).
// One value per thread, fp32, no fast-math, contraction off: every fused operation is an explicit fmaf, so host and device agree.
//
// The arithmetic restates the step kernels' scalar code in its operation order -- Fast::sphere_box_dist (pbre_fast.hpp),
// Shapes::sphere_round and Shapes::candidate (pbre_objstep.hpp), Core::sphere_hull (pbre_core.hpp) -- without the normals and contact
// points a solver needs; the rule set is model/contacts.py: contact_flags.
//
// Hull early-out.  A piece whose bounding sphere is farther from the collision sphere than `reach` contributes that lower bound
// (|p - centre| - radius - sr) and its faces are not visited, as in Core::sphere_hull.  The query passes reach = margin + the largest
// bounding radius of the pieces: the smallest distance over spheres and pieces is then exact wherever it is below that reach (so wherever
// it is below margin), and a lower bound that is itself >= margin above it.
#pragma once
#include <cmath>
#include "pbre_math.hpp"
#include "pbre_tables.hpp"
PBRE_FP_CONTRACT_OFF

namespace pbre {
namespace cq {

constexpr float CQ_FAR = 3.0e38f;        // PBRE_CQ_FAR

static PBRE_HD float dot3(const float* a, const float* b) { return fmaf(a[0], b[0], fmaf(a[1], b[1], a[2] * b[2])); }
// R^T (s - c): world -> the frame of the body at c with rotation R (row major, body -> world)
static PBRE_HD void to_local(const float* R, const float* s, const float* c, float* dl) {
    const float d[3] = {s[0] - c[0], s[1] - c[1], s[2] - c[2]};
    dl[0] = fmaf(R[0], d[0], fmaf(R[3], d[1], R[6] * d[2]));
    dl[1] = fmaf(R[1], d[0], fmaf(R[4], d[1], R[7] * d[2]));
    dl[2] = fmaf(R[2], d[0], fmaf(R[5], d[1], R[8] * d[2]));
}
static PBRE_HD float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// sphere (centre in the box frame dl, radius sr) against the box |x| <= h: Fast::sphere_box_dist
static PBRE_HD float sphere_box_local(const float* dl, float sr, const float* h) {
    const float df[3] = {dl[0] - clampf(dl[0], -h[0], h[0]), dl[1] - clampf(dl[1], -h[1], h[1]), dl[2] - clampf(dl[2], -h[2], h[2])};
    const float len = sqrtf(dot3(df, df));
    const float best = fminf(fminf(h[0] - fabsf(dl[0]), h[1] - fabsf(dl[1])), h[2] - fabsf(dl[2]));
    return len < 1e-9f ? -best - sr : len - sr;
}
static PBRE_HD float sphere_box_dist(const float* sc, float sr, const float* bc, const float* R, const float* h) {
    float dl[3];
    to_local(R, sc, bc, dl);
    return sphere_box_local(dl, sr, h);
}
// ... against an axis-aligned box (the table): R = I, for which R^T d = d exactly
static PBRE_HD float sphere_aabb_dist(const float* sc, float sr, const float* bc, const float* h) {
    const float dl[3] = {sc[0] - bc[0], sc[1] - bc[1], sc[2] - bc[2]};
    return sphere_box_local(dl, sr, h);
}

// ... against a round object (shape 1: sphere of radius h[0]; 2: cylinder about local z, radius h[0], half height h[2]): the distance of
// Shapes::sphere_round, with its rule for a centre inside the cylinder: rho <= radius and |z| <= half height, not only a closest point
// closer than 1e-9 -- in fp32 (dl - u rho) leaves a residue of that size for a centre well inside
static PBRE_HD float sphere_round_dist(int shape, const float* sc, float sr, const float* c, const float* R, const float* h) {
    if (shape == 1) {
        const float d[3] = {sc[0] - c[0], sc[1] - c[1], sc[2] - c[2]};
        return sqrtf(dot3(d, d)) - h[0] - sr;
    }
    float dl[3];
    to_local(R, sc, c, dl);
    const float rho = sqrtf(fmaf(dl[0], dl[0], dl[1] * dl[1]));
    const bool ax0 = !(rho > 1e-12f);
    const float ir = 1.f / fmaxf(rho, 1e-30f);
    const float ux = ax0 ? 1.f : dl[0] * ir, uy = ax0 ? 0.f : dl[1] * ir;
    const float rc = fminf(rho, h[0]), zc = fminf(fmaxf(dl[2], -h[2]), h[2]);
    const float df[3] = {dl[0] - ux * rc, dl[1] - uy * rc, dl[2] - zc};
    const float len = sqrtf(dot3(df, df));
    const float er = h[0] - rho, ez = h[2] - fabsf(dl[2]);
    if (len >= 1e-9f && !(er >= 0.f && ez >= 0.f)) return len - sr;
    return er <= ez ? -er - sr : -ez - sr;
}

// ... against one convex piece given as nf triangles (a[3], ab[3], ac[3], unit outward normal[3]) in the frame of p: the largest face-plane
// distance when p is behind every face (inside), else the closest point over the triangles (Ericson, Real-Time Collision Detection 5.1.5,
// with selects in the priority order of its early returns: vertex A, B, edge AB, vertex C, edge AC, BC, face) -- Core::sphere_hull
static PBRE_HD float sphere_piece_dist(const float* Tf, int nf, const float* p, float sr) {
    float best2 = 3e38f, maxsd = -3e38f;
#pragma unroll 1
    for (int f = 0; f < nf; f++) {
        const float* T = Tf + 12 * f;
        const float* ab = T + 3;
        const float* ac = T + 6;
        const float ap[3] = {p[0] - T[0], p[1] - T[1], p[2] - T[2]};
        const float sd = dot3(T + 9, ap);
        maxsd = sd > maxsd ? sd : maxsd;
        const float d1 = dot3(ab, ap), d2 = dot3(ac, ap);
        const float bp[3] = {ap[0] - ab[0], ap[1] - ab[1], ap[2] - ab[2]}, cp[3] = {ap[0] - ac[0], ap[1] - ac[1], ap[2] - ac[2]};
        const float d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
        const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
        const float den = 1.f / (va + vb + vc);
        float v = vb * den, w = vc * den;                                                   // face interior
        const float e43 = d4 - d3, e56 = d5 - d6;
        if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) { const float wbc = e43 / (e43 + e56); v = 1.f - wbc; w = wbc; }
        if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { v = 0.f; w = d2 / (d2 - d6); }
        if (d6 >= 0.f && d5 <= d6) { v = 0.f; w = 1.f; }
        if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { v = d1 / (d1 - d3); w = 0.f; }
        if (d3 >= 0.f && d4 <= d3) { v = 1.f; w = 0.f; }
        if (d1 <= 0.f && d2 <= 0.f) { v = 0.f; w = 0.f; }
        const float e[3] = {p[0] - (T[0] + (ab[0] * v + ac[0] * w)), p[1] - (T[1] + (ab[1] * v + ac[1] * w)), p[2] - (T[2] + (ab[2] * v + ac[2] * w))};
        const float e2 = dot3(e, e);
        best2 = e2 < best2 ? e2 : best2;                                                    // (a NaN from a degenerate triangle's 0 / 0 never wins)
    }
    return maxsd <= 0.f ? maxsd - sr : sqrtf(best2) - sr;
}

// the largest bounding-sphere radius of the pieces of the hull table H (pbre_tables.hpp)
static PBRE_HD float hull_rb_max(const float* H) {
    const int np = (int)H[0];
    float rb = 0.f;
    for (int q = 0; q < np; q++) rb = fmaxf(rb, H[HULL_D0 + HULL_DP * q + 7]);
    return rb;
}
// ... against the hull or compound of table H: the nearest piece; p: the sphere's centre in the object's frame.  See "Hull early-out".
static PBRE_HD float sphere_hull_dist(const float* H, const float* p, float sr, float reach) {
    const int np = (int)H[0];
    float best = CQ_FAR;
#pragma unroll 1
    for (int q = 0; q < np; q++) {
        const float* D = H + HULL_D0 + HULL_DP * q;
        const float e[3] = {p[0] - D[4], p[1] - D[5], p[2] - D[6]};
        const float far = sqrtf(dot3(e, e)) - D[7] - sr;
        const float d = far < reach ? sphere_piece_dist(H + HULL_T0 + 12 * (int)D[1], (int)D[3], p, sr) : far;
        best = fminf(best, d);
    }
    return best;
}

// a robot sphere against the object, whatever its shape (PBRE_SHAPE_*); op, Ro: the object's position and rotation
static PBRE_HD float sphere_object_dist(int shape, const float* sc, float sr, const float* op, const float* Ro, const float* oh, const float* H, float reach) {
    if (shape == 0) return sphere_box_dist(sc, sr, op, Ro, oh);
    if (shape == 3) {
        float p[3];
        to_local(Ro, sc, op, p);
        return sphere_hull_dist(H, p, sr, reach);
    }
    return sphere_round_dist(shape, sc, sr, op, Ro, oh);
}

// one candidate point (offset r from the object's centre, world axes) against the table top: z - top where the point lies over the top in
// x and y and above the underside, else CQ_FAR
static PBRE_HD float candidate_dist(const float* op, float rx, float ry, float rz, const float* tc, const float* th) {
    const float x = op[0] + rx, y = op[1] + ry, z = op[2] + rz;
    const bool on = fabsf(x - tc[0]) <= th[0] && fabsf(y - tc[1]) <= th[1] && z > tc[2] - th[2];
    return on ? z - (tc[2] + th[2]) : CQ_FAR;
}
// the object against the table: the smallest candidate_dist over the shape's candidate points (Shapes::candidate's slots; a hull: every
// vertex of every piece), CQ_FAR when none counts
static PBRE_HD float object_table_dist(int shape, const float* op, const float* R, const float* h, const float* H, const float* tc, const float* th) {
    float best = CQ_FAR;
    if (shape == 3) {
        const int np = (int)H[0];
#pragma unroll 1
        for (int q = 0; q < np; q++) {
            const float* D = H + HULL_D0 + HULL_DP * q;
            const float* V = H + HULL_V0 + 4 * (int)D[0];
            const int nv = (int)D[2];
#pragma unroll 1
            for (int i = 0; i < nv; i++) {
                const float* l = V + 4 * i;
                best = fminf(best, candidate_dist(op, fmaf(R[0], l[0], fmaf(R[1], l[1], R[2] * l[2])), fmaf(R[3], l[0], fmaf(R[4], l[1], R[5] * l[2])),
                                                  fmaf(R[6], l[0], fmaf(R[7], l[1], R[8] * l[2])), tc, th));
            }
        }
        return best;
    }
    if (shape == 1) return candidate_dist(op, 0.f, 0.f, -h[0], tc, th);
    for (int v = 0; v < 8; v++) {
        float lx, ly, lz;
        if (shape == 0) { lx = (v & 1) ? h[0] : -h[0]; ly = (v & 2) ? h[1] : -h[1]; lz = (v & 4) ? h[2] : -h[2]; }
        else {
            const float s = v < 4 ? -1.f : 1.f;
            const int k = v & 3;
            if (k < 3) {
                const float cs = k == 0 ? 1.f : -0.5f, sn = k == 0 ? 0.f : (k == 1 ? 0.86602540378443865f : -0.86602540378443865f);
                lx = h[0] * cs; ly = h[0] * sn; lz = s * h[2];
            } else {                                 // the rim's lowest point; unused while the axis is vertical
                const float dx = -R[6], dy = -R[7];
                const float len = sqrtf(fmaf(dx, dx, dy * dy));
                if (!(len >= 1e-6f)) continue;
                lx = h[0] * dx / len; ly = h[0] * dy / len; lz = s * h[2];
            }
        }
        best = fminf(best, candidate_dist(op, fmaf(R[0], lx, fmaf(R[1], ly, R[2] * lz)), fmaf(R[3], lx, fmaf(R[4], ly, R[5] * lz)),
                                          fmaf(R[6], lx, fmaf(R[7], ly, R[8] * lz)), tc, th));
    }
    return best;
}

// rotation (row major) of the quaternion x, y, z, w as stored, not renormalised (model/contacts.py: _quat_R)
static PBRE_HD void quat_R(const float* q, float* R) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - w * z); R[2] = 2.f * (x * z + w * y);
    R[3] = 2.f * (x * y + w * z); R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - w * x);
    R[6] = 2.f * (x * z - w * y); R[7] = 2.f * (y * z + w * x); R[8] = 1.f - 2.f * (x * x + y * y);
}

}  // namespace cq
}  // namespace pbre
PBRE_FP_CONTRACT_FAST
