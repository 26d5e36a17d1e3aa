// CPU check of the episode time limit (mgym_config::max_episode_steps): the decision header modurl_gym_amd/csrc/time_limit.h and
// LunarLander's per-env step / reset source (ll_*.h) compiled for the host, as tests/native/ll_host_check.cpp does.  Built and run by
// tests/test_time_limit_host.py, which compares every word written here with the CPU oracle inside its Python time-limit wrapper
// (tests/time_limit_ref.py); no GPU involved.  This is a test of the kernel logic, not a product CPU path.
//   time_limit_check ll <n> <limit> <steps> <seed> <out>   n LunarLander envs, wind on, uniform actions (LCG), reset-on-finish
//       (finished = done | truncated, as under MGYM_FLAG_AUTO_RESET).  <out>: reset observation [8][n] f32, then per step
//       actions [n] u32, obs [8][n] f32, reward [n] f32, done [n] u8, truncated [n] u8, elapsed-after [n] u32.
//   time_limit_check rule <limit> <set_value> <steps>      MountainCar's 16-bit counter: set (clamped), then <steps> x advance + compare.
//       Prints the stored value after the set, then "truncated elapsed" per step.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#include "../../modurl_gym_amd/csrc/time_limit.h"
#include "../../modurl_gym_amd/csrc/ll_free.h"
using namespace mgym;

static int run_rule(int argc, char** argv) {
    if (argc < 5) return 2;
    const uint32_t limit = (uint32_t)strtoul(argv[2], 0, 0), set = (uint32_t)strtoul(argv[3], 0, 0);
    const int steps = atoi(argv[4]);
    uint32_t el = (uint16_t)tl_clamp(set);   // what mountaincar_set_elapsed_kernel stores
    printf("%u\n", el);
    for (int t = 0; t < steps; ++t) {        // what the TL kernels do per env-step, through the 16-bit column
        el = (uint16_t)tl_advance(el);
        printf("%u %u\n", tl_truncated(limit, el), el);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "rule")) return run_rule(argc, argv);
    if (argc < 7 || strcmp(argv[1], "ll")) { fprintf(stderr, "usage: see the head of time_limit_check.cpp\n"); return 2; }
    const uint64_t n = strtoull(argv[2], 0, 0);
    const uint32_t limit = (uint32_t)strtoul(argv[3], 0, 0);
    const int steps = atoi(argv[4]);
    const uint64_t seed = strtoull(argv[5], 0, 0);
    FILE* out = fopen(argv[6], "wb");
    if (!out) return 2;
    LLDev d;
    memset(&d, 0, sizeof d);
    d.n = n; d.n_pad = (n + 1023) / 1024 * 1024; d.seed = seed; d.env_id_base = 0;
    std::vector<uint32_t> st((size_t)ll_state_words(d.n_pad), 0u);
    std::vector<float> obsbuf((size_t)8 * d.n_pad, 0.0f);
    d.st = st.data(); d.obs = obsbuf.data();
    ll_make_const(d.k, -10.0f, 1, 15.0f, 1.5f);
    d.k.max_steps = limit;
    d.kd = &d.k;
    PolyTab tab;
    for (int p = 0; p < 2; ++p) { tab.count[p] = d.k.poly_count[p]; for (int q = 0; q < kMaxPoly; ++q) { tab.v[p][q] = d.k.poly_v[p][q]; tab.n[p][q] = d.k.poly_n[p][q]; } }
    WorldTmp h_tmp;
    uint32_t h_hot[3 * kSlots]; const CtHot hot{h_hot, 1u, 1u};
    VConstraint h_vc[kSlots]; PConstraint h_pc[kSlots];
    CSolverMem mem; mem.vc = h_vc; mem.vc_stride = 1; mem.vc_near = kSlots; mem.vc_far = nullptr; mem.vc_far_stride = 0; mem.pc = h_pc; mem.pc_stride = 1; mem.cap = kSlots;
    std::vector<float> obs(8 * n), rew(n);
    std::vector<uint8_t> done(n), trunc(n);
    std::vector<uint32_t> act(n), elapsed(n);
    for (uint64_t i = 0; i < n; ++i) {
        World w; EnvRegs e; float state[8];
        w.t = &h_tmp;
        ll_load(d, i, w, e, hot);
        ll_env_reset(d, i, w, e, tab, mem, state);
        ll_store(d, i, w, e);
        for (int q = 0; q < 8; ++q) obs[q * n + i] = state[q];
    }
    fwrite(obs.data(), 4, obs.size(), out);
    uint32_t rs = (uint32_t)seed * 2654435761u + 12345u;
    unsigned long overflow = 0;
    for (int t = 0; t < steps; ++t) {
        for (uint64_t i = 0; i < n; ++i) { rs = rs * 1664525u + 1013904223u; act[i] = (rs >> 16) & 3u; }
        for (uint64_t i = 0; i < n; ++i) {
            float state[8], reward, d0, d1; uint32_t dn = 0u, tr = 0u, el = 0u;
            bool fast = false;
            // the dispatch of ll_free_pass / ll_contact_body, and the lines they run after a finished step
            if (ll_free_eligible(ST(C_FLAGS))) {
                FreeRegs f; EnvRegs e;
                ll_free_load(d, i, f, e);
                ll_dispersion(d, i, e, d0, d1);
                uint32_t moved;
                if (ll_free_env_step(d, i, f, e, tab, act[i], d0, d1, state, reward, dn, moved) == FREE_DONE) {
                    ll_free_store(d, i, f, e);
                    tr = ll_truncated(d, e); el = tl_ll_elapsed(e.step);
                    fast = true;
                }
            }
            if (!fast) {
                World w; EnvRegs e;
                w.t = &h_tmp;
                ll_load(d, i, w, e, hot);
                ll_dispersion(d, i, e, d0, d1);
                ll_env_step(w, e, tab, d.k, mem, act[i], d0, d1, state, reward, dn);
                if (w.overflow) overflow++;
                ll_store(d, i, w, e);
                tr = ll_truncated(d, e); el = tl_ll_elapsed(e.step);
            }
            if (dn | tr) {   // auto-reset: finished = done | truncated; the step's observation is the reset's
                World w; EnvRegs e;
                w.t = &h_tmp;
                ll_load(d, i, w, e, hot);
                ll_env_reset(d, i, w, e, tab, mem, state);
                ll_store(d, i, w, e);
                el = tl_ll_elapsed(e.step);
            }
            for (int q = 0; q < 8; ++q) obs[q * n + i] = state[q];
            rew[i] = reward; done[i] = (uint8_t)dn; trunc[i] = (uint8_t)tr; elapsed[i] = el;
        }
        fwrite(act.data(), 4, n, out); fwrite(obs.data(), 4, obs.size(), out); fwrite(rew.data(), 4, n, out);
        fwrite(done.data(), 1, n, out); fwrite(trunc.data(), 1, n, out); fwrite(elapsed.data(), 4, n, out);
    }
    fclose(out);
    printf("envs=%lu steps=%d limit=%u overflow=%lu\n", (unsigned long)n, steps, limit, overflow);
    return overflow ? 1 : 0;
}
