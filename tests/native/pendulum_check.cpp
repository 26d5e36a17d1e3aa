// CPU check of Pendulum-v1: modurl_gym_amd/csrc/pendulum_step.h — the per-environment lines the kernels of pendulum.hip run (step, time limit, reset
// draw, the uniform / linear / hidden-layer policies) — compiled for the host with g++ -ffp-contract=off and driven by the loop the kernels put round
// them.  Built and run by tests/test_pendulum_host.py (tests/pendulum_ref.py), which compares every word with a numpy restatement of the text of
// include/mgym.h; no GPU involved.  This is a test of the kernel logic, not a product CPU path.
//   shared object:  pendulum_run(..) below
//   program:        pendulum_check   runs a fixed scenario through pendulum_run (every policy, imported states, a NaN action) and prints one
//                   checksum line per case; it is also what a sanitizer build runs (it has its own main and reads no input)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define __host__
#include "../../modurl_gym_amd/csrc/pendulum_step.h"
using namespace mgym;

// flush = 1: the x86 flush-to-zero and denormals-are-zero bits (MXCSR 15 and 6) are set for the duration of the run and restored after it: what a
// build that flushes denormals would compute, for the check that the edge cases of tests/classic_edge_cases.py would notice one
#if defined(__x86_64__) || defined(__i386__)
#include <xmmintrin.h>
struct FlushScope {
    unsigned saved;
    bool on;
    explicit FlushScope(bool flush) : saved(_mm_getcsr()), on(flush) { if (on) _mm_setcsr(saved | 0x8040u); }
    ~FlushScope() { if (on) _mm_setcsr(saved); }
    static bool supported() { return true; }
};
#else
struct FlushScope {
    explicit FlushScope(bool) {}
    static bool supported() { return false; }
};
#endif

enum { POL_TABLE = 0, POL_LINEAR = 1, POL_UNIFORM = 2, POL_MLP_RELU = 3, POL_MLP_TANH = 4 };

struct PdRun {
    uint64_t n; int32_t steps; uint64_t seed, env_id_base; float g; uint32_t limit; int32_t auto_reset;
    int32_t policy; const float* weights; int32_t hidden; uint64_t policy_seed; uint32_t call;
    const uint32_t* actions_in;   // [steps][n] f32 words (POL_TABLE)
    const uint32_t* state_in;     // [3][n] th, thdot, episode; NULL: reset() every env from the created state
    uint32_t* actions_out;        // [steps][n]
    float *obs0, *obs, *reward;   // [3][n], [steps][3][n], [steps][n]
    uint8_t* trunc;               // [steps][n]
    uint32_t *elapsed_out, *state_out;   // [n], [3][n]
    uint64_t finished;            // truncated env-steps (mgym_episode_count)
    int32_t bad;                  // a NaN action was seen (the sticky MGYM_ERR_INVALID_ACTION)
    int32_t flush;                // run with denormals flushed to zero (inputs and results); 0 in every other use
};

template <bool TL>
static void run(PdRun& p) {
    const uint64_t n = p.n;
    const float c_g = pendulum_c_g(p.g);
    std::vector<float> th(n, 0.0f), td(n, 0.0f), cs(n, 1.0f), sn(n, 0.0f);
    std::vector<uint32_t> ep(n, 0u), el(n, 0u), a(n, 0u);
    for (uint64_t i = 0; i < n; ++i) {
        if (p.state_in) {   // pendulum_import_kernel
            th[i] = as_f32(p.state_in[i]); td[i] = as_f32(p.state_in[n + i]); ep[i] = p.state_in[2 * n + i];
            pendulum_sincos(th[i], cs[i], sn[i]);
        } else {            // pendulum_reset_kernel
            pendulum_reset_one(p.seed, p.env_id_base + i, ep[i], th[i], td[i], cs[i], sn[i]);
            ep[i] += 1u;
        }
        el[i] = 0u;
        p.obs0[i] = cs[i]; p.obs0[n + i] = sn[i]; p.obs0[2 * n + i] = td[i];
    }
    MlpPack<3, 1> pack;
    PdLinearPolicy lin{};
    if (p.policy == POL_MLP_RELU || p.policy == POL_MLP_TANH) mlp_pack<3, 1>(p.weights, p.hidden, pack);
    if (p.policy == POL_LINEAR) lin = PdLinearPolicy{{p.weights[0], p.weights[1], p.weights[2]}, p.weights[3]};
    p.finished = 0; p.bad = 0;
    const uint32_t no_word[1] = {0u};   // (the greedy head reads no word)
    for (int t = 0; t < p.steps; ++t) {
        // the action of every env from what it holds before the step (pendulum_rollout_kernel)
        if (p.policy == POL_UNIFORM) {
            for (uint64_t i0 = 0; i0 < n; i0 += 4) {
                uint32_t a4[4];
                pendulum_uniform_actions(p.policy_seed, p.call, p.env_id_base + i0, (uint32_t)t, a4);
                for (int k = 0; k < 4; ++k) a[i0 + k] = a4[k];
            }
        } else {
            for (uint64_t i = 0; i < n; ++i) {
                const float o[1][3] = {{cs[i], sn[i], td[i]}};
                uint32_t a1[1];
                if (p.policy == POL_LINEAR) a1[0] = pendulum_linear_action(lin, cs[i], sn[i], td[i]);
                else if (p.policy == POL_MLP_RELU) mlp_actions<3, 1, MLP_ACT_RELU, MLP_HEAD_GREEDY, 1>(pack, o, no_word, 0.0f, a1);
                else if (p.policy == POL_MLP_TANH) mlp_actions<3, 1, MLP_ACT_TANH, MLP_HEAD_GREEDY, 1>(pack, o, no_word, 0.0f, a1);
                else a1[0] = p.actions_in[(uint64_t)t * n + i];
                a[i] = a1[0];
            }
        }
        for (uint64_t i = 0; i < n; ++i) {
            float r;
            uint32_t tr;
            if (!pendulum_env_step<TL>(c_g, p.limit, th[i], td[i], cs[i], sn[i], el[i], a[i], r, tr)) p.bad = 1;
            p.finished += tr;
            if (p.auto_reset && tr) {   // pendulum_reset_env
                pendulum_reset_one(p.seed, p.env_id_base + i, ep[i], th[i], td[i], cs[i], sn[i]);
                ep[i] += 1u; el[i] = 0u;
            }
            const uint64_t off = (uint64_t)t * n + i;
            p.actions_out[off] = a[i]; p.reward[off] = r; p.trunc[off] = (uint8_t)tr;
            float* o = p.obs + (uint64_t)t * 3 * n + i;
            o[0] = cs[i]; o[n] = sn[i]; o[2 * n] = td[i];
        }
    }
    for (uint64_t i = 0; i < n; ++i) {
        p.elapsed_out[i] = el[i];
        p.state_out[i] = as_u32(th[i]); p.state_out[n + i] = as_u32(td[i]); p.state_out[2 * n + i] = ep[i];
    }
}

extern "C" {

int pendulum_run(PdRun* p) {
    if (!p || (p->policy == POL_UNIFORM && (p->n % 4 || p->env_id_base % 4)) || p->limit > kMaxEpisodeSteps) return 1;
    if (p->flush && !FlushScope::supported()) return 2;
    const FlushScope scope(p->flush != 0);
    if (p->limit) run<true>(*p); else run<false>(*p);
    return 0;
}

}  // extern "C"

// ---- the program: a fixed scenario, one checksum line per case (sum of the output words, mod 2^64) ----
static uint64_t sum_words(const void* p, size_t words) {
    uint64_t s = 0;
    for (size_t i = 0; i < words; ++i) { uint32_t w; memcpy(&w, static_cast<const char*>(p) + 4 * i, 4); s += w; }
    return s;
}

int main() {
    const uint64_t n = 256;
    const int steps = 64;
    std::vector<uint32_t> acts((size_t)steps * n), acts_out((size_t)steps * n), elapsed(n), state(3 * n), imported(3 * n, 0u);
    std::vector<float> obs0(3 * n), obs((size_t)steps * 3 * n), rew((size_t)steps * n), w(64 * 4 + 65);
    std::vector<uint8_t> trunc((size_t)steps * n);
    uint32_t rs = 12345u;
    auto next = [&rs]() { rs = rs * 1664525u + 1013904223u; return rs; };
    for (auto& v : acts) v = as_u32((float)(next() >> 8) * (5.0f / 16777216.0f) - 2.5f);   // [-2.5, 2.5)
    acts[5] = 0x7fc00000u;   // a NaN action
    for (auto& v : w) v = (float)(next() >> 8) * (2.0f / 16777216.0f) - 1.0f;
    const float big[] = {1e6f, -1e6f, 12345.678f, 3.1415927f, -3.1415927f, -0.0f};
    for (uint64_t i = 0; i < n; ++i) { imported[i] = as_u32(big[i % 6]); imported[n + i] = as_u32((float)(i % 17) - 8.0f); imported[2 * n + i] = (uint32_t)i; }
    int rc = 0;
    for (int c = 0; c < 7; ++c) {
        PdRun p{};
        p.n = n; p.steps = steps; p.seed = 0x1234567811ull; p.env_id_base = 1024; p.g = 10.0f; p.limit = c == 6 ? 0u : 7u; p.auto_reset = c != 5;
        p.policy = c < 5 ? c : POL_TABLE; p.weights = w.data(); p.hidden = 33; p.policy_seed = 99; p.call = 2;
        p.actions_in = acts.data(); p.state_in = c >= 5 ? imported.data() : nullptr;
        p.actions_out = acts_out.data(); p.obs0 = obs0.data(); p.obs = obs.data(); p.reward = rew.data(); p.trunc = trunc.data();
        p.elapsed_out = elapsed.data(); p.state_out = state.data();
        rc |= pendulum_run(&p);
        uint64_t ts = 0;
        for (uint8_t v : trunc) ts += v;
        printf("case %d actions %llu obs0 %llu obs %llu reward %llu truncated %llu elapsed %llu state %llu finished %llu bad %d\n", c,
               (unsigned long long)sum_words(acts_out.data(), acts_out.size()), (unsigned long long)sum_words(obs0.data(), obs0.size()),
               (unsigned long long)sum_words(obs.data(), obs.size()), (unsigned long long)sum_words(rew.data(), rew.size()), (unsigned long long)ts,
               (unsigned long long)sum_words(elapsed.data(), elapsed.size()), (unsigned long long)sum_words(state.data(), state.size()),
               (unsigned long long)p.finished, p.bad);
    }
    return rc;
}
