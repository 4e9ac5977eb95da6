// Stand-alone run of the reset sequence's recording executor (reset_seq_host.cpp), of make_motor_cmd and of the motor-record writers
// (csrc/pbre_host.hpp) under AddressSanitizer and UBSan (the Makefile's flags).  Every buffer is a heap block of exactly the size the
// callee may use -- the record list as long as the sequence, a motor record of 4 W floats, 64 commanded joints -- so an index past one is
// a heap overflow.  Exits 0 and prints "reset_seq_san OK" when no sanitizer report fired and the results obey the functions' own rules.
#include <cstdio>
#include <memory>
#include <vector>
#include "pbre_host.hpp"
#include "pbre_reset_seq.hpp"

using namespace pbre;
extern "C" int reset_seq_record(const int* in, int* out, int cap, int* rc);

template <class S>
static bool writers(int& checked) {
    std::unique_ptr<TablesT<S>> T(new TablesT<S>());
    std::memset(T.get(), 0, sizeof *T);
    for (int l = 0; l < S::W; l++) { T->home[l] = 0.01f * l; T->kp_hold[l] = 0.2f; T->kp_act[l] = 0.5f; T->lower[l] = -1.f; T->upper[l] = 1.f; T->act_idx[l] = l < S::NJ ? S::NJ - 1 - l : -1; }
    std::vector<float> m((size_t)4 * S::W, -9.f), act((size_t)S::NJ, 3.f);
    for (int l = 0; l < S::W; l++) mrec_init<S>(*T, m.data(), l);
    for (int l = 0; l < S::W; l++) if (m[l] != T->home[l] || m[S::W + l] != 0.2f || m[2 * S::W + l] != 1.f || m[3 * S::W + l] != 0.f) return false;
    for (int l = 0; l < S::W; l++) mrec_cmd_joint<S>(*T, m.data(), l, act.data(), 0.7f);
    for (int l = 0; l < S::W; l++) if (m[l] != (l < S::NJ ? 1.f : T->home[l]) || m[3 * S::W + l] != (l < S::NJ ? 0.7f : 0.f)) return false;      // clipped to the upper limit
    std::vector<int32_t> dofs(64);
    std::vector<float> tg(64);
    for (int k = 0; k < 64; k++) { dofs[k] = k % S::NJ; tg[k] = 0.1f * k; }
    pbre_physics ph;
    default_physics(ph);
    std::unique_ptr<MotorCmd> cmd(new MotorCmd);
    if (make_motor_cmd(*cmd, 64, dofs.data(), tg.data(), 0.3, 10.0, 1.0, S::NJ, ph) != nullptr) return false;
    for (int k = 0; k < 64; k++) mrec_set<S>(m.data(), *cmd, k);
    if (m[S::W + dofs[63]] != 0.3f || m[3 * S::W + dofs[63]] != 1.f) return false;
    if (make_motor_cmd(*cmd, 65, dofs.data(), tg.data(), 0.3, 10.0, 1.0, S::NJ, ph) == nullptr) return false;      // refused before anything is read
    dofs[63] = S::NJ;
    if (make_motor_cmd(*cmd, 64, dofs.data(), tg.data(), 0.3, 0.0, 0.0, S::NJ, ph) == nullptr) return false;
    if (make_motor_cmd(*cmd, 0, nullptr, nullptr, 0.3, 0.0, 0.0, S::NJ, ph) != nullptr || cmd->fscale != 1.f || cmd->vmax != 0.f) return false;
    checked += 5;
    return true;
}

int main() {
    int checked = 0;
    for (int robot = 0; robot < 3; robot++) for (int ik = 0; ik < 2; ik++) for (int task = 0; task < 3; task++) for (int mrec = 0; mrec < 2; mrec++) for (int fl = 0; fl < 4; fl++) {
        int in[6] = {robot, ik, task, mrec, fl, -1}, rc = 0;
        const int len = reset_seq_record(in, nullptr, 0, &rc);
        if (rc != 0 || len < 4 || len > 7) { std::printf("sequence of %d operations, rc %d\n", len, rc); return 1; }
        for (int fail = -1; fail < len; fail++) {
            std::vector<int> out((size_t)3 * len);
            in[5] = fail;
            const int got = reset_seq_record(in, out.data(), len, &rc);
            if (got != (fail < 0 ? len : fail + 1) || rc != (fail < 0 ? 0 : -7)) { std::printf("fail_at %d: %d operations, rc %d\n", fail, got, rc); return 1; }
            checked++;
        }
    }
    if (!writers<Shape128>(checked) || !writers<ShapePA>(checked) || !writers<ShapeIA>(checked)) { std::printf("a motor-record writer broke its rule\n"); return 1; }
    std::printf("reset_seq_san OK (%d runs)\n", checked);
    return 0;
}
