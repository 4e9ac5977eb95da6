// pbre_camera.hpp -- per-ray functions of the camera (include/pbre_camera.h): ray against capsule, box, cylinder, convex face planes and
// the floor, and the shading.  PBRE_HD as in pbre_math.hpp: the same header compiles for the device (pbre_camera.hip) and for the host
// (tests/camera_host).  fp32, no fast-math.
//
// A ray is o + t d with d NOT normalised: the camera scales d so that d . (view axis) = 1, which makes t the depth along the view axis.
// Every primitive is convex, so a ray meets it in one interval [t_in, t_out]; a function returns t_in (the entry root) or CAM_MISS.  The
// caller counts a hit only for near <= t_in <= far, so a ray that starts inside a primitive (t_in < 0) does not see it.
#pragma once
#include <cmath>
#ifndef PBRE_HD
#define PBRE_HD
#endif

namespace pbre {
namespace cam {

constexpr float CAM_MISS = -1.0f;        // (any t_in <= 0 is a miss for the caller; this is the value for "no interval at all")
constexpr float CAM_BIG = 3.0e38f;

static PBRE_HD float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// interval of the ball |x - c| <= r (oc = o - c, dd = d . d); false: none
static PBRE_HD bool ball_interval(const float* oc, const float* d, float dd, float r, float& t0, float& t1) {
    const float b = dot3(oc, d), c = dot3(oc, oc) - r * r;
    const float h = b * b - dd * c;
    if (!(h >= 0.0f)) return false;
    const float s = sqrtf(h);
    t0 = (-b - s) / dd; t1 = (-b + s) / dd;
    return true;
}

// Capsule: all points within r of the segment a-b = ball(a) U ball(b) U the solid cylinder between the end planes.  The union is convex, so
// its interval starts at the smallest start of the three.  Exact; no case needs a near-parallel ray to pick "the" cap.  a == b: a sphere.
static PBRE_HD float ray_capsule(const float* o, const float* d, const float* a, const float* b, float r) {
    const float dd = dot3(d, d);
    const float oa[3] = {o[0] - a[0], o[1] - a[1], o[2] - a[2]};
    float t0, t1, tin = CAM_BIG;
    if (ball_interval(oa, d, dd, r, t0, t1)) tin = t0;
    const float ba[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const float baba = dot3(ba, ba);
    if (baba > 0.0f) {
        const float ob[3] = {o[0] - b[0], o[1] - b[1], o[2] - b[2]};
        if (ball_interval(ob, d, dd, r, t0, t1)) tin = fminf(tin, t0);
        // solid cylinder: the infinite one, |x - a|^2 baba - ((x - a) . ba)^2 <= r^2 baba, cut by 0 <= (x - a) . ba <= baba
        const float bard = dot3(ba, d), baoa = dot3(ba, oa), rdoa = dot3(d, oa), oaoa = dot3(oa, oa);
        const float A = baba * dd - bard * bard, B = baba * rdoa - baoa * bard, Cc = baba * oaoa - baoa * baoa - r * r * baba;
        float c0 = -CAM_BIG, c1 = CAM_BIG;
        bool ok = true;
        if (A > 0.0f) {
            const float h = B * B - A * Cc;
            if (h >= 0.0f) { const float s = sqrtf(h); c0 = (-B - s) / A; c1 = (-B + s) / A; } else ok = false;
        } else ok = Cc <= 0.0f;                      // parallel to the axis: inside the infinite cylinder or never
        if (ok) {
            if (bard > 0.0f) { c0 = fmaxf(c0, -baoa / bard); c1 = fminf(c1, (baba - baoa) / bard); }
            else if (bard < 0.0f) { c0 = fmaxf(c0, (baba - baoa) / bard); c1 = fminf(c1, -baoa / bard); }
            else ok = baoa >= 0.0f && baoa <= baba;
            if (ok && c0 <= c1) tin = fminf(tin, c0);
        }
    }
    return tin < CAM_BIG ? tin : CAM_MISS;
}
// outward unit normal of the capsule at the surface point x: away from the nearest point of the segment
static PBRE_HD void capsule_normal(const float* x, const float* a, const float* b, float* n) {
    const float ba[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, xa[3] = {x[0] - a[0], x[1] - a[1], x[2] - a[2]};
    const float baba = dot3(ba, ba);
    const float y = baba > 0.0f ? fminf(fmaxf(dot3(xa, ba) / baba, 0.0f), 1.0f) : 0.0f;
    float v[3] = {xa[0] - y * ba[0], xa[1] - y * ba[1], xa[2] - y * ba[2]};
    const float l = sqrtf(dot3(v, v));
    if (l > 0.0f) { n[0] = v[0] / l; n[1] = v[1] / l; n[2] = v[2] / l; } else { n[0] = 0.0f; n[1] = 0.0f; n[2] = 1.0f; }
}

// Box |x - c| <= h per axis, in the frame o and d are given in (slabs).  A ray parallel to a slab is inside it when |o - c| <= h (a ray
// along a face is inside).  n: the entry face's outward normal.
static PBRE_HD float ray_box(const float* o, const float* d, const float* c, const float* h, float* n) {
    float tin = -CAM_BIG, tout = CAM_BIG;
    float m[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 3; k++) {
        const float oc = o[k] - c[k];
        if (d[k] != 0.0f) {
            const float ta = (-h[k] - oc) / d[k], tb = (h[k] - oc) / d[k];
            const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
            if (lo > tin) { tin = lo; m[0] = m[1] = m[2] = 0.0f; m[k] = d[k] > 0.0f ? -1.0f : 1.0f; }
            tout = fminf(tout, hi);
        } else if (fabsf(oc) > h[k]) return CAM_MISS;
    }
    if (!(tin <= tout)) return CAM_MISS;
    n[0] = m[0]; n[1] = m[1]; n[2] = m[2];
    return tin;
}

// Cylinder about z through the origin of the frame o and d are given in: x^2 + y^2 <= r^2, |z| <= hz
static PBRE_HD float ray_cylinder(const float* o, const float* d, float r, float hz, float* n) {
    const float A = d[0] * d[0] + d[1] * d[1], B = o[0] * d[0] + o[1] * d[1], Cc = o[0] * o[0] + o[1] * o[1] - r * r;
    float c0 = -CAM_BIG, c1 = CAM_BIG;
    if (A > 0.0f) {
        const float h = B * B - A * Cc;
        if (!(h >= 0.0f)) return CAM_MISS;
        const float s = sqrtf(h);
        c0 = (-B - s) / A; c1 = (-B + s) / A;
    } else if (Cc > 0.0f) return CAM_MISS;
    float s0 = -CAM_BIG, s1 = CAM_BIG;
    if (d[2] != 0.0f) {
        const float ta = (-hz - o[2]) / d[2], tb = (hz - o[2]) / d[2];
        s0 = fminf(ta, tb); s1 = fmaxf(ta, tb);
    } else if (fabsf(o[2]) > hz) return CAM_MISS;
    const float tin = fmaxf(c0, s0), tout = fminf(c1, s1);
    if (!(tin <= tout)) return CAM_MISS;
    if (s0 > c0) { n[0] = 0.0f; n[1] = 0.0f; n[2] = d[2] > 0.0f ? -1.0f : 1.0f; }
    else { n[0] = (o[0] + tin * d[0]) / r; n[1] = (o[1] + tin * d[1]) / r; n[2] = 0.0f; }
    return tin;
}

// Convex body as `count` face planes: plane f passes through pt + f * stride with unit outward normal nm + f * stride.  Entry = the
// largest t over the planes with n . d < 0, exit = the smallest over n . d > 0; a plane parallel to the ray with the origin outside: miss.
static PBRE_HD float ray_planes(const float* o, const float* d, const float* pt, const float* nm, int stride, int count, float* n) {
    float tin = -CAM_BIG, tout = CAM_BIG;
    int fi = -1;
#pragma unroll 1
    for (int f = 0; f < count; f++) {
        const float* a = pt + f * stride;
        const float* m = nm + f * stride;
        const float den = dot3(m, d);
        const float dist = m[0] * (o[0] - a[0]) + m[1] * (o[1] - a[1]) + m[2] * (o[2] - a[2]);      // > 0: outside this face
        if (den < 0.0f) { const float t = -dist / den; if (t > tin) { tin = t; fi = f; } }
        else if (den > 0.0f) tout = fminf(tout, -dist / den);
        else if (dist > 0.0f) return CAM_MISS;
    }
    if (fi < 0 || !(tin <= tout)) return CAM_MISS;
    const float* m = nm + fi * stride;
    n[0] = m[0]; n[1] = m[1]; n[2] = m[2];
    return tin;
}

// does the ray's line meet the ball (c, r) at all?  (the hull pieces' bounding spheres)
static PBRE_HD bool ray_meets_ball(const float* o, const float* d, const float* c, float r) {
    const float oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
    const float b = dot3(oc, d);
    return b * b - dot3(d, d) * (dot3(oc, oc) - r * r) >= 0.0f;
}

// Floor: the half space z <= z0, seen from above only.  Normal +z.
static PBRE_HD float ray_floor(const float* o, const float* d, float z0) {
    if (!(d[2] < 0.0f)) return CAM_MISS;
    return (z0 - o[2]) / d[2];
}

// one colour channel: floor(255 base (ambient + (1 - ambient) max(0, n . l)) + 0.5), clamped to 0..255
static PBRE_HD int shade(float base, float ndotl, float ambient) {
    const float v = 255.0f * base * (ambient + (1.0f - ambient) * fmaxf(0.0f, ndotl));
    return (int)fminf(fmaxf(floorf(v + 0.5f), 0.0f), 255.0f);
}

}  // namespace cam
}  // namespace pbre
