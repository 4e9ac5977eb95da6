// Stand-alone run of the solve of csrc/pbre_ik.hpp under AddressSanitizer and UBSan (the Makefile's flags).  Arguments: files holding a
// RobotTable each (raw float64, as model/table.py builds them; tests/test_ik_host.py writes the iCub with hands and the floating-base
// iCub).  Every table is solved for a few envs with random start values towards the pose of a perturbed configuration: the chain to the
// table's ee_link in both problem sizes, then the chain to the last link (a fingertip of the hands model: torso, arm and finger) position
// only, with and without a mask and limits; the working block is exactly as large as the device's, so an index past it is a heap overflow.
// Exits 0 and prints "ik_san OK" when no sanitizer report fired, every output is finite and the iteration counts are within the cap.
#include <cmath>
#include <cstdio>
#include <vector>
#include "ik_run.hpp"

static unsigned rng_state = 2463534242u;
static float urand() { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) / 16777216.0f; }

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: ik_san table.f64 ...\n"); return 2; }
    int checked = 0;
    for (int a = 1; a < argc; a++) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) { std::printf("cannot open %s\n", argv[a]); return 2; }
        std::vector<double> t;
        double x;
        while (std::fread(&x, sizeof x, 1, f) == 1) t.push_back(x);
        std::fclose(f);
        if (t.size() < 24 || t[0] != 1346523717.0 || t.size() < (size_t)(24 + (int)t[2] * 40)) { std::printf("%s: not a RobotTable\n", argv[a]); return 2; }
        const int nl = (int)t[2], nd = (int)t[3], ee = (int)t[4], n = 70;        // (70 envs: the columns wrap around once)
        if (nl > 128 || nd > 64) { std::printf("%s: table too large\n", argv[a]); return 2; }
        std::vector<float> qs((size_t)n * nd), tp((size_t)n * 3), tq((size_t)n * 4);
        for (auto& v : qs) v = 0.6f * (urand() - 0.5f);
        for (int e = 0; e < n; e++) {
            tp[3 * e] = 0.3f + 0.2f * urand(); tp[3 * e + 1] = 0.4f * (urand() - 0.5f); tp[3 * e + 2] = 0.7f + 0.3f * urand();
            for (int k = 0; k < 4; k++) tq[4 * e + k] = 2.0f * (urand() - 0.5f) + (k == 3 ? 1.5f : 0.0f);      // not normalised
        }
        std::vector<uint8_t> mask(nd > 0 ? nd : 1, 0);
        for (int d = 0; d < nd; d += 2) mask[d] = 1;
        int longest = 0;
        for (int variant = 0; variant < 5; variant++) {
            ik_host::Query Q;
            Q.link = variant < 2 ? ee : nl - 1;
            Q.q_start = qs.data(); Q.target_pos = tp.data();
            Q.target_quat = (variant == 0 || variant == 4) ? tq.data() : nullptr;
            Q.dof_mask = variant == 3 ? mask.data() : nullptr;
            Q.clamp = variant >= 3;
            Q.max_iters = variant == 4 ? 0 : 25;
            Q.residual = variant == 1 ? 0.0f : 1e-3f;
            Q.point[0] = 0.01f; Q.point[1] = -0.02f; Q.point[2] = 0.03f;
            std::vector<float> q((size_t)n * nd), err((size_t)n * 2);
            std::vector<int32_t> it(n, -1);
            Q.q = q.data(); Q.err = variant == 2 ? nullptr : err.data(); Q.iters = it.data();
            pbre::ik::Chain ch;
            if (pbre::ik::resolve_chain(t.data(), Q.link, Q.dof_mask, ch) != 0 || ik_host::run(t.data(), n, Q) != 0) { std::printf("%s: chain too long\n", argv[a]); return 1; }
            if (ch.nm > longest) longest = ch.nm;
            for (float v : q) if (!std::isfinite(v)) { std::printf("%s variant %d: a non-finite q\n", argv[a], variant); return 1; }
            if (Q.err) for (float v : err) if (!std::isfinite(v) || v < 0.0f) { std::printf("%s variant %d: a bad error\n", argv[a], variant); return 1; }
            for (int e = 0; e < n; e++) {
                if (it[e] < 0 || it[e] > Q.max_iters || (variant == 1 && it[e] != 25)) { std::printf("%s variant %d: %d iterations\n", argv[a], variant, it[e]); return 1; }
                if (variant == 4) for (int d = 0; d < nd; d++) if (q[(size_t)e * nd + d] != qs[(size_t)e * nd + d]) { std::printf("%s: max_iters = 0 moved a joint\n", argv[a]); return 1; }
            }
            checked++;
        }
        std::printf("%s: %d links, %d DoF, longest chain %d moving DoFs\n", argv[a], nl, nd, longest);
    }
    std::printf("ik_san OK (%d queries)\n", checked);
    return 0;
}
