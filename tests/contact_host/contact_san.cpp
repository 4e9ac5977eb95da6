// Stand-alone run of the hull and compound functions of csrc/pbre_contacts.hpp under AddressSanitizer and UBSan (the Makefile's flags):
// hull tables of 1 and 4 pieces with 4 and 32 vertices per piece, built by the engine's builder (csrc/pbre_host.hpp: build_hull), queried
// from a grid of sphere centres inside, near and far outside the early-out reach, and as an object lying on and hanging over a table.
// Exits 0 and prints "contact_san OK" when no sanitizer report fired and the results obey the functions' own bounds.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "pbre_host.hpp"
#include "pbre_contacts.hpp"

using namespace pbre;

static unsigned rng_state = 12345u;
static double urand() { rng_state = rng_state * 1664525u + 1013904223u; return (double)(rng_state >> 8) / 16777216.0; }

// nv points on a sphere of radius r about c (convex position: every one is a hull vertex); nv = 4: a tetrahedron
static void piece(std::vector<double>& v, int nv, const double* c, double r) {
    if (nv == 4) {
        const double t[4][3] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
        for (auto& x : t) for (int k = 0; k < 3; k++) v.push_back(c[k] + r * x[k] / std::sqrt(3.0));
        return;
    }
    for (int i = 0; i < nv; i++) {           // a spiral: no four coplanar, at most 2 nv - 4 = 60 triangles
        const double z = 1.0 - 2.0 * (i + 0.5) / nv, rho = std::sqrt(1.0 - z * z), a = 2.399963229728653 * i + 0.01 * urand();
        const double x[3] = {rho * std::cos(a), rho * std::sin(a), z};
        for (int k = 0; k < 3; k++) v.push_back(c[k] + r * x[k]);
    }
}

int main() {
    const double NaN = std::nan("");
    int checked = 0;
    for (int np : {1, 4}) for (int nv : {4, 32}) {
        std::vector<double> v;
        for (int p = 0; p < np; p++) {
            if (p) for (int k = 0; k < 3; k++) v.push_back(NaN);
            const double c[3] = {np == 1 ? 0.0 : 0.05 * (p - 1.5), np == 1 ? 0.0 : 0.01 * p, 0.0};
            piece(v, nv, c, 0.03);
        }
        auto H = std::make_unique<HullTable>();
        const std::string e = build_hull(v.data(), (int)v.size() / 3, *H);
        if (!e.empty()) { std::printf("build_hull(%d pieces, %d vertices): %s\n", np, nv, e.c_str()); return 1; }
        // the table exactly as large as the builder filled it: a read past the last triangle is a heap overflow
        const size_t used = HULL_T0 + 12 * (size_t)H->nf;
        std::vector<float> T(H->data, H->data + used);
        if (H->nv != np * nv) { std::printf("vertex count %d\n", H->nv); return 1; }
        const float rb = cq::hull_rb_max(T.data()), margin = 0.001f;
        for (int i = 0; i < 4000; i++) {
            const float scale = i % 4 == 0 ? 0.02f : (i % 4 == 1 ? 0.1f : 1.0f);
            const float p[3] = {scale * (float)(2 * urand() - 1), scale * (float)(2 * urand() - 1), scale * (float)(2 * urand() - 1)};
            const float sr = 0.01f * (float)urand();
            const float d_exact = cq::sphere_hull_dist(T.data(), p, sr, cq::CQ_FAR);
            const float d_early = cq::sphere_hull_dist(T.data(), p, sr, margin + rb);
            if (!(d_early <= d_exact) || !std::isfinite(d_exact)) { std::printf("lower bound violated: %g > %g\n", d_early, d_exact); return 1; }
            if (d_exact < margin + rb && d_early != d_exact) { std::printf("not exact below the reach: %g vs %g\n", d_early, d_exact); return 1; }
            if (d_exact >= margin && d_early < margin) { std::printf("a bound below the margin: %g\n", d_early); return 1; }
            checked++;
        }
        const float tc[3] = {0.85f, 0.0f, 0.6f}, th[3] = {0.75f, 0.5f, 0.025f}, oh[3] = {0.1f, 0.1f, 0.1f};
        for (int i = 0; i < 200; i++) {
            const float q[4] = {(float)(urand() - 0.5), (float)(urand() - 0.5), (float)(urand() - 0.5), 0.5f + (float)urand()};
            const float n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            const float qn[4] = {q[0] / n, q[1] / n, q[2] / n, q[3] / n};
            float R[9];
            cq::quat_R(qn, R);
            const float op[3] = {i % 2 ? 0.1f + 0.02f * (float)urand() : 0.5f, 0.0f, 0.625f + 0.05f * (float)urand()};      // odd: over the table's edge at x = 0.1
            const float d = cq::object_table_dist(3, op, R, oh, T.data(), tc, th);
            if (!(d > -0.2f)) { std::printf("object-table distance %g\n", d); return 1; }
            checked++;
        }
    }
    std::printf("contact_san OK (%d queries)\n", checked);
    return 0;
}
