// The per-pair functions of csrc/pbre_contacts.hpp behind a C interface, one call per array of spheres or object poses
// (tests/test_contact_host.py), and the engine's own hull table builder (csrc/pbre_host.hpp: build_hull) for their hull arguments.
#include "pbre_host.hpp"
#include "pbre_contacts.hpp"

using namespace pbre;

extern "C" {

int cq_hull_floats() { return HULL_FLOATS; }
// verts: [n][3], a compound's pieces separated by rows of three NaNs; out: HULL_FLOATS floats.  0, or 1 when the builder refuses the set
int cq_build_hull(const double* verts, int n, float* out) {
    static HullTable H;
    if (!build_hull(verts, n, H).empty()) return 1;
    for (int i = 0; i < HULL_FLOATS; i++) out[i] = H.data[i];
    return 0;
}
float cq_hull_rb_max(const float* H) { return cq::hull_rb_max(H); }
// spheres sc[n][3], sr[n] against the object (shape, position op, rotation Ro row major, half extents oh, hull table H)
void cq_sphere_object(int n, int shape, const float* sc, const float* sr, const float* op, const float* Ro, const float* oh, const float* H, float reach, float* out) {
    for (int i = 0; i < n; i++) out[i] = cq::sphere_object_dist(shape, sc + 3 * i, sr[i], op, Ro, oh, H, reach);
}
void cq_sphere_table(int n, const float* sc, const float* sr, const float* tc, const float* th, float* out) {
    for (int i = 0; i < n; i++) out[i] = cq::sphere_aabb_dist(sc + 3 * i, sr[i], tc, th);
}
// object poses pose[n][7] (position, quaternion x y z w) against the table top
void cq_object_table(int n, int shape, const float* pose, const float* oh, const float* H, const float* tc, const float* th, float* out) {
    for (int i = 0; i < n; i++) {
        float R[9];
        cq::quat_R(pose + 7 * i + 3, R);
        out[i] = cq::object_table_dist(shape, pose + 7 * i, R, oh, H, tc, th);
    }
}

}
