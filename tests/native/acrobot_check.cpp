// CPU check of Acrobot-v1: modurl_gym_amd/csrc/acrobot_step.h — the per-environment lines the kernels of acrobot.hip run (the RK4 step, time limit,
// reset draws, the uniform / linear / hidden-layer / sampled policies) — compiled for the host with g++ -ffp-contract=off and driven by the loop the
// kernels put round them.  Built and run by tests/test_acrobot_host.py (tests/acrobot_ref.py), which compares every word with a numpy restatement of
// the text of include/mgym.h; no GPU involved.  This is a test of the kernel logic, not a product CPU path.
//   shared object:  acrobot_run(..) below (the restatement's libm calls in bulk are those of tests/native/pendulum_check.cpp)
//   program:        acrobot_check   runs a fixed scenario through acrobot_run (every policy, imported states that terminate at once, that never
//                   settle, an infinity, a NaN, an invalid action) and prints one checksum line per case; it is also what a sanitizer build runs
//                   (it has its own main and reads no input)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define __host__
#include "../../modurl_gym_amd/csrc/acrobot_step.h"
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

enum { POL_TABLE = 0, POL_LINEAR = 1, POL_UNIFORM = 2, POL_MLP_RELU = 3, POL_MLP_TANH = 4, POL_MLP_RELU_SAMPLE = 5, POL_MLP_TANH_SAMPLE = 6 };

struct AbRun {
    uint64_t n; int32_t steps; uint64_t seed, env_id_base; uint32_t limit; int32_t auto_reset;
    int32_t policy; const float* weights; int32_t hidden; uint64_t policy_seed; uint32_t call;
    const uint32_t* actions_in;   // [steps][n] u32 words (POL_TABLE)
    const uint32_t* state_in;     // [5][n] th1, th2, w1, w2, episode; NULL: reset() every env from the created state
    uint32_t* actions_out;        // [steps][n]
    float *obs0, *obs, *reward;   // [6][n], [steps][6][n], [steps][n]
    uint8_t *done, *trunc;        // [steps][n]
    uint32_t *elapsed_out, *state_out;   // [n], [5][n]
    uint64_t finished;            // env-steps with done | truncated (mgym_episode_count)
    int32_t bad;                  // an action above 2 was seen (the sticky MGYM_ERR_INVALID_ACTION)
    int32_t flush;                // run with denormals flushed to zero (inputs and results); 0 in every other use
};

template <bool TL>
static void run(AbRun& p) {
    const uint64_t n = p.n;
    std::vector<AbEnv> e(n);
    std::vector<uint32_t> ep(n, 0u), el(n, 0u), a(n, 0u);
    for (uint64_t i = 0; i < n; ++i) {
        if (p.state_in) {   // acrobot_import_kernel
            e[i].th1 = as_f32(p.state_in[i]); e[i].th2 = as_f32(p.state_in[n + i]); e[i].w1 = as_f32(p.state_in[2 * n + i]); e[i].w2 = as_f32(p.state_in[3 * n + i]);
            ep[i] = p.state_in[4 * n + i];
            acrobot_trig(e[i]);
        } else {            // acrobot_reset_kernel
            acrobot_reset_one(p.seed, p.env_id_base + i, ep[i], e[i]);
            ep[i] += 1u;
        }
        float o[6];
        acrobot_obs(e[i], o);
        for (int c = 0; c < 6; ++c) p.obs0[c * n + i] = o[c];
    }
    MlpPack<6, 3> pack;
    AbLinearPolicy lin{};
    const bool mlp = p.policy >= POL_MLP_RELU;
    const bool tanh_act = p.policy == POL_MLP_TANH || p.policy == POL_MLP_TANH_SAMPLE, samples = p.policy >= POL_MLP_RELU_SAMPLE;
    if (mlp) mlp_pack<6, 3>(p.weights, p.hidden, pack);
    if (p.policy == POL_LINEAR)
        for (int j = 0; j < 3; ++j) {
            for (int q = 0; q < 6; ++q) lin.w[j][q] = p.weights[7 * j + q];
            lin.b[j] = p.weights[7 * j + 6];
        }
    p.finished = 0; p.bad = 0;
    Philox4 bits{};
    for (int t = 0; t < p.steps; ++t) {
        // the action of every env from what it holds before the step (acrobot_rollout_kernel)
        for (uint64_t i0 = 0; i0 < n; i0 += 4) {
            Philox4 w{};
            if (p.policy == POL_UNIFORM) bits = acrobot_uniform_block(p.policy_seed, p.call, p.env_id_base + i0, (uint32_t)t);   // (the kernel keeps the even step's block)
            if (samples) w = env_draw(p.policy_seed, p.env_id_base + i0, p.call, SLOT_POLICY_SAMPLE + (uint32_t)t);
            for (uint64_t i = i0; i < i0 + 4 && i < n; ++i) {
                float o[1][6];
                acrobot_obs(e[i], o[0]);
                uint32_t a1[1];
                const uint32_t w1[1] = {w.w[i - i0]};
                if (p.policy == POL_UNIFORM) a1[0] = acrobot_uniform_action(bits.w[i - i0], (uint32_t)t);
                else if (p.policy == POL_LINEAR) a1[0] = acrobot_linear_action(lin, o[0]);
                else if (samples && tanh_act) mlp_actions<6, 3, MLP_ACT_TANH, MLP_HEAD_SAMPLE, 1>(pack, o, w1, 0.0f, a1);
                else if (samples) mlp_actions<6, 3, MLP_ACT_RELU, MLP_HEAD_SAMPLE, 1>(pack, o, w1, 0.0f, a1);
                else if (mlp && tanh_act) mlp_actions<6, 3, MLP_ACT_TANH, MLP_HEAD_GREEDY, 1>(pack, o, w1, 0.0f, a1);
                else if (mlp) mlp_actions<6, 3, MLP_ACT_RELU, MLP_HEAD_GREEDY, 1>(pack, o, w1, 0.0f, a1);
                else a1[0] = p.actions_in[(uint64_t)t * n + i];
                a[i] = a1[0];
            }
        }
        for (uint64_t i = 0; i < n; ++i) {
            float r;
            uint32_t dn, tr;
            if (!acrobot_env_step<TL>(p.limit, e[i], el[i], a[i], r, dn, tr)) p.bad = 1;
            const uint64_t off = (uint64_t)t * n + i;
            float* o = p.obs + (uint64_t)t * 6 * n + i;
            p.finished += dn | tr;
            if (p.auto_reset && (dn | tr)) {   // acrobot_reset_env
                acrobot_reset_one(p.seed, p.env_id_base + i, ep[i], e[i]);
                ep[i] += 1u; el[i] = 0u;
            }
            p.actions_out[off] = a[i]; p.reward[off] = r; p.done[off] = (uint8_t)dn; p.trunc[off] = (uint8_t)tr;
            float ow[6];
            acrobot_obs(e[i], ow);
            for (int c = 0; c < 6; ++c) o[c * n] = ow[c];
        }
    }
    for (uint64_t i = 0; i < n; ++i) {
        p.elapsed_out[i] = el[i];
        p.state_out[i] = as_u32(e[i].th1); p.state_out[n + i] = as_u32(e[i].th2); p.state_out[2 * n + i] = as_u32(e[i].w1); p.state_out[3 * n + i] = as_u32(e[i].w2);
        p.state_out[4 * n + i] = ep[i];
    }
}

extern "C" int acrobot_run(AbRun* p) {
    const bool draws = p && (p->policy == POL_UNIFORM || p->policy >= POL_MLP_RELU_SAMPLE);
    if (!p || (draws && (p->n % 4 || p->env_id_base % 4)) || p->limit > kMaxEpisodeSteps) return 1;
    if (p->flush && !FlushScope::supported()) return 2;
    const FlushScope scope(p->flush != 0);
    if (p->limit) run<true>(*p); else run<false>(*p);
    return 0;
}

// ---- the program: a fixed scenario, one checksum line per case (sum of the output words, mod 2^64) ----
static uint64_t sum_words(const void* p, size_t words) {
    uint64_t s = 0;
    for (size_t i = 0; i < words; ++i) { uint32_t w; memcpy(&w, static_cast<const char*>(p) + 4 * i, 4); s += w; }
    return s;
}

int main() {
    const uint64_t n = 256;
    const int steps = 64;
    std::vector<uint32_t> acts((size_t)steps * n), acts_out((size_t)steps * n), elapsed(n), state(5 * n), imported(5 * n, 0u);
    std::vector<float> obs0(6 * n), obs((size_t)steps * 6 * n), rew((size_t)steps * n), w(64 * 7 + 3 * 65);
    std::vector<uint8_t> done((size_t)steps * n), trunc((size_t)steps * n);
    uint32_t rs = 12345u;
    auto next = [&rs]() { rs = rs * 1664525u + 1013904223u; return rs; };
    for (auto& v : acts) v = (next() >> 8) % 3u;
    acts[5] = 3u;   // an invalid action
    for (auto& v : w) v = (float)(next() >> 8) * (2.0f / 16777216.0f) - 1.0f;
    // imported states: terminating at once (th1 = pi), hanging, fast beyond the clamps, far outside [-pi, pi], an infinity and a NaN
    const float th1s[] = {3.14159274f, 0.0f, 2.0f, 1e6f, INFINITY, 0.5f, -3.14159274f, 1000.0f};
    const float th2s[] = {0.0f, 0.0f, -1.0f, -12345.678f, 0.25f, NAN, 0.0f, -0.0f};
    const float w1s[] = {0.0f, 0.0f, 13.0f, -12.0f, 1.0f, 0.0f, 1.0f, 1e30f};
    const float w2s[] = {0.0f, 0.0f, -29.0f, 28.0f, 0.0f, 1.0f, -1.0f, -1e30f};
    for (uint64_t i = 0; i < n; ++i) {
        imported[i] = as_u32(th1s[i % 8]); imported[n + i] = as_u32(th2s[i % 8]); imported[2 * n + i] = as_u32(w1s[i % 8]); imported[3 * n + i] = as_u32(w2s[i % 8]);
        imported[4 * n + i] = (uint32_t)i;
    }
    int rc = 0;
    for (int c = 0; c < 9; ++c) {
        AbRun p{};
        p.n = n; p.steps = steps; p.seed = 0x1234567811ull; p.env_id_base = 1024; p.limit = c == 8 ? 0u : 7u; p.auto_reset = c != 7;
        p.policy = c < 7 ? c : POL_TABLE; p.weights = w.data(); p.hidden = 33; p.policy_seed = 99; p.call = 2;
        p.actions_in = acts.data(); p.state_in = c >= 7 ? imported.data() : nullptr;
        p.actions_out = acts_out.data(); p.obs0 = obs0.data(); p.obs = obs.data(); p.reward = rew.data(); p.done = done.data(); p.trunc = trunc.data();
        p.elapsed_out = elapsed.data(); p.state_out = state.data();
        rc |= acrobot_run(&p);
        uint64_t ts = 0, ds = 0;
        for (uint8_t v : trunc) ts += v;
        for (uint8_t v : done) ds += v;
        printf("case %d actions %llu obs0 %llu obs %llu reward %llu done %llu truncated %llu elapsed %llu state %llu finished %llu bad %d\n", c,
               (unsigned long long)sum_words(acts_out.data(), acts_out.size()), (unsigned long long)sum_words(obs0.data(), obs0.size()),
               (unsigned long long)sum_words(obs.data(), obs.size()), (unsigned long long)sum_words(rew.data(), rew.size()), (unsigned long long)ds,
               (unsigned long long)ts, (unsigned long long)sum_words(elapsed.data(), elapsed.size()), (unsigned long long)sum_words(state.data(), state.size()),
               (unsigned long long)p.finished, p.bad);
    }
    return rc;
}
