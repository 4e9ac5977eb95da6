// Stand-alone run of the walks of csrc/pbre_kin.hpp under AddressSanitizer and UBSan (the Makefile's flags).  Arguments: files holding a
// RobotTable each (raw float64, as model/table.py builds them; tests/test_kin_host.py writes the iCub with hands -- 62 links, 60 DoF, the
// largest -- and the floating-base iCub with its prismatic joints).  Every table goes through every function for a few envs with random
// joint states, every output and option, the column buffers exactly as large as the device's: an index past a buffer is a heap overflow.
// Exits 0 and prints "kin_san OK" when no sanitizer report fired, every output is finite and M is symmetric with a positive diagonal.
#include <cmath>
#include <cstdio>
#include <vector>
#include "kin_run.hpp"

static unsigned rng_state = 2463534242u;
static float urand() { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) / 16777216.0f; }

static bool finite_all(const std::vector<float>& v) { for (float x : v) if (!std::isfinite(x)) return false; return true; }

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: kin_san table.f64 ...\n"); return 2; }
    int checked = 0;
    for (int a = 1; a < argc; a++) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) { std::printf("cannot open %s\n", argv[a]); return 2; }
        std::vector<double> t;
        double x;
        while (std::fread(&x, sizeof x, 1, f) == 1) t.push_back(x);
        std::fclose(f);
        if (t.size() < 24 || t[0] != 1346523717.0 || t.size() < (size_t)(24 + (int)t[2] * 40)) { std::printf("%s: not a RobotTable\n", argv[a]); return 2; }
        const int nl = (int)t[2], nd = (int)t[3], n = 5;
        if (nl > pbre::kin::MAX_LINKS || nd > pbre::kin::MAX_DOF) { std::printf("%s: table too large\n", argv[a]); return 2; }
        const int W = nd <= 9 ? 16 : (nd <= 20 ? 32 : (nd <= 32 ? 64 : 128)), stride = 2 * W + 16;
        int prismatic = 0;
        for (int i = 0; i < nl; i++) prismatic += t[24 + i * 40 + 1] == 2.0;
        std::vector<float> state((size_t)n * stride, 0.0f), qdd((size_t)n * nd);
        for (int e = 0; e < n; e++) for (int d = 0; d < nd; d++) {
            state[(size_t)e * stride + d] = 0.6f * (urand() - 0.5f);
            state[(size_t)e * stride + W + d] = 2.0f * (urand() - 0.5f);
            qdd[(size_t)e * nd + d] = 6.0f * (urand() - 0.5f);
        }
        for (int variant = 0; variant < 3; variant++) {
            std::vector<int32_t> links;
            if (variant == 0) for (int i = 0; i < nl; i++) links.push_back(i);
            if (variant == 1) { links.push_back(nl - 1); links.push_back(0); links.push_back(nl - 1); }
            const size_t nq = links.size();
            std::vector<float> pose(nq * 7 * n), vel(nq * 6 * n), jac((size_t)6 * nd * n), mass((size_t)nd * nd * n), tau((size_t)nd * n);
            kin_host::Query q;
            q.n_links = (int)nq; q.links = links.data(); q.at_com = variant == 1; q.jac_at_com = variant == 2;
            q.jac_link = variant == 0 ? (int)t[4] : nl - 1;
            q.jac_point[0] = 0.01f; q.jac_point[1] = -0.02f; q.jac_point[2] = 0.03f;
            q.qdd = variant == 2 ? nullptr : qdd.data();
            q.pose = nq ? pose.data() : nullptr; q.vel = nq && variant != 1 ? vel.data() : nullptr;
            q.jac = jac.data(); q.mass = variant != 1 ? mass.data() : nullptr; q.tau = variant != 2 ? tau.data() : nullptr;
            kin_host::run(t.data(), n, state.data(), stride, W, 9.8f, q);
            if ((q.pose && !finite_all(pose)) || (q.vel && !finite_all(vel)) || !finite_all(jac) || (q.mass && !finite_all(mass)) || (q.tau && !finite_all(tau))) {
                std::printf("%s variant %d: a non-finite output\n", argv[a], variant); return 1;
            }
            if (q.mass) for (int e = 0; e < n; e++) for (int i = 0; i < nd; i++) {
                const float* M = mass.data() + (size_t)e * nd * nd;
                if (!(M[i * nd + i] > 0.0f)) { std::printf("%s: M[%d][%d] = %g\n", argv[a], i, i, M[i * nd + i]); return 1; }
                for (int j = 0; j < i; j++) if (M[i * nd + j] != M[j * nd + i]) { std::printf("%s: M not symmetric at %d %d\n", argv[a], i, j); return 1; }
            }
            if (q.pose) for (size_t r = 0; r < nq * n; r++) {
                const float* p = pose.data() + r * 7;
                const float nn = p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6];
                if (!(std::fabs(nn - 1.0f) < 1e-4f) || p[6] < 0.0f) { std::printf("%s: quaternion norm %g w %g\n", argv[a], nn, p[6]); return 1; }
            }
            checked++;
        }
        std::printf("%s: %d links, %d DoF, %d prismatic\n", argv[a], nl, nd, prismatic);
    }
    std::printf("kin_san OK (%d queries)\n", checked);
    return 0;
}
