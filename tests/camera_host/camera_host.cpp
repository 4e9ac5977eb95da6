// The per-ray functions of csrc/pbre_camera.hpp behind a C interface, one call per array of rays (tests/test_camera_host.py).
// Rays: o[n][3], d[n][3]; results: t[n] (the entry root, or a value <= 0 / CAM_MISS for a miss), nrm[n][3] where the function gives one.
#include "pbre_camera.hpp"

using namespace pbre::cam;

extern "C" {

void cam_capsule(int n, const float* o, const float* d, const float* a, const float* b, float r, float* t, float* nrm) {
    for (int i = 0; i < n; i++) {
        t[i] = ray_capsule(o + 3 * i, d + 3 * i, a, b, r);
        const float x[3] = {o[3 * i] + t[i] * d[3 * i], o[3 * i + 1] + t[i] * d[3 * i + 1], o[3 * i + 2] + t[i] * d[3 * i + 2]};
        capsule_normal(x, a, b, nrm + 3 * i);
    }
}
void cam_box(int n, const float* o, const float* d, const float* c, const float* h, float* t, float* nrm) {
    for (int i = 0; i < n; i++) t[i] = ray_box(o + 3 * i, d + 3 * i, c, h, nrm + 3 * i);
}
void cam_cylinder(int n, const float* o, const float* d, float r, float hz, float* t, float* nrm) {
    for (int i = 0; i < n; i++) t[i] = ray_cylinder(o + 3 * i, d + 3 * i, r, hz, nrm + 3 * i);
}
// planes: count records of 6 floats, a point of the plane and its unit outward normal
void cam_planes(int n, const float* o, const float* d, const float* planes, int count, float* t, float* nrm) {
    for (int i = 0; i < n; i++) t[i] = ray_planes(o + 3 * i, d + 3 * i, planes, planes + 3, 6, count, nrm + 3 * i);
}
void cam_floor(int n, const float* o, const float* d, float z0, float* t) {
    for (int i = 0; i < n; i++) t[i] = ray_floor(o + 3 * i, d + 3 * i, z0);
}
void cam_shade(int n, const float* base, const float* ndotl, float ambient, int* out) {
    for (int i = 0; i < n; i++) out[i] = shade(base[i], ndotl[i], ambient);
}

}
