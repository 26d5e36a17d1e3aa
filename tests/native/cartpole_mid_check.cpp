// CartPole's kernel source (modurl_gym_amd/csrc/cartpole_step.h, compiled for the host) against the CPU oracle, which calls
// glibc, at given pole angles: every <is_euler, sutton_barto> variant, four small theta_dot, K steps with alternating actions
// (no reset: a pole past the threshold keeps spinning, cartpole.rs:319-335).  Each step takes the path the step kernel takes:
// the fast form when cartpole_fast_ok() admits the state, else the reference form.  Run by tests/test_sincos_mid_range.py with
// the angles of tests/sincos_mid_range.py.  Usage: cartpole_mid_check <K> <angle> ...  (angles as C hex floats)
// Prints "checked=<steps> mismatches=<m>"; exit code 0 iff m is 0.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../modurl_gym_amd/csrc/cartpole_step.h"
extern "C" {
#include "../../oracle/oracle.h"
}
using namespace mgym;

template <bool EULER, bool SB>
static void step_kernel_form(const CartPoleParams& p, float* s, uint32_t& ctr, uint32_t a, float& r, uint32_t& d, uint32_t& t) {
    if (cartpole_fast_ok(s[2], s[3], a)) cartpole_step_fast<EULER, SB>(p, s[0], s[1], s[2], s[3], ctr, a, r, d, t);
    else cartpole_step_ref(p, s[0], s[1], s[2], s[3], ctr, a, r, d, t);
}

template <bool EULER, bool SB>
static void run(int K, const float* angles, int na, unsigned long& checked, unsigned long& bad) {
    const CartPoleParams p = cartpole_params(EULER ? 1 : 0, SB ? 1 : 0);
    const float thetadots[4] = {0.0f, 1e-3f, -0.05f, 0.3f};
    for (int i = 0; i < na; ++i) {
        for (int j = 0; j < 4; ++j) {
            for (uint32_t a0 = 0; a0 < 2; ++a0) {
                ora_cartpole o;
                ora_cartpole_new(&o, SB ? 1 : 0, EULER ? 1 : 0);
                const float init[4] = {0.25f, -0.125f, angles[i], thetadots[j]};
                memcpy(o.state, init, sizeof init);
                o.steps_since_reset = 0; o.sbt_is_some = 0; o.sbt = 0;
                float s[4];
                memcpy(s, init, sizeof init);
                uint32_t ctr = cp_ctr_pack(0u, 0u, 0u);
                for (int k = 0; k < K; ++k) {
                    const uint32_t a = (a0 + (uint32_t)k) & 1u;
                    ora_stepinfo info;
                    ora_cartpole_step(&o, a, &info);
                    float r; uint32_t d, t;
                    step_kernel_form<EULER, SB>(p, s, ctr, a, r, d, t);
                    bool same = as_u32(r) == as_u32(info.reward) && d == info.done && t == info.truncated;
                    for (int q = 0; q < 4; ++q) same = same && as_u32(s[q]) == as_u32(o.state[q]);
                    ++checked;
                    if (!same) {
                        if (bad < 8) printf("<euler %d, sb %d> theta0 %a theta_dot0 %a step %d: kernel (%a %a %a %a) r %a d %u | oracle (%a %a %a %a) r %a d %u\n",
                                            (int)EULER, (int)SB, angles[i], thetadots[j], k, s[0], s[1], s[2], s[3], r, d,
                                            o.state[0], o.state[1], o.state[2], o.state[3], info.reward, (unsigned)info.done);
                        ++bad;
                        break;   // the trajectories have parted: later steps say nothing new
                    }
                }
            }
        }
    }
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <K> <angle>...\n", argv[0]); return 2; }
    const int K = atoi(argv[1]);
    const int na = argc - 2;
    float* angles = (float*)malloc(sizeof(float) * (size_t)na);
    for (int i = 0; i < na; ++i) angles[i] = strtof(argv[2 + i], nullptr);
    unsigned long checked = 0, bad = 0;
    run<true, false>(K, angles, na, checked, bad);
    run<true, true>(K, angles, na, checked, bad);
    run<false, false>(K, angles, na, checked, bad);
    run<false, true>(K, angles, na, checked, bad);
    printf("checked=%lu mismatches=%lu\n", checked, bad);
    free(angles);
    return bad ? 1 : 0;
}
