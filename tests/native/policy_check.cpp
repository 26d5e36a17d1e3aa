// CPU check of the hidden-layer policies' action call: mlp_actions<D, A, ACT, HEAD, N>(net, o, w, sigma, act) of modurl_gym_amd/csrc/mlp_policy.h over both
// nets (mlp_policy.h's MlpPack, mlp2_policy.h's Mlp2Net) — the lines the rollout kernels compile — built with g++ -ffp-contract=off (tests/policy_header.py).
//   as a shared object: policy_eval(D, A, depth, act, head, H1, H2, policy, sigma, n, stride, obs [D][stride], words, actions [n], scores [n][A] or NULL)
//     depth   1 (policy: W1[H1][D], b1, W2[A][H1], b2; H2 is ignored) or 2 (W1[H1][D], b1, W2[H2][H1], b2, W3[A][H2], b3; no MLP_ACT_TANH)
//     head    MLP_HEAD_GREEDY  the argmax (A > 1) or the bits of the one score (A = 1); words are not read
//             MLP_HEAD_SAMPLE  the categorical draw (A > 1): words [n], one Philox word per environment
//             MLP_HEAD_GAUSS   the Gaussian draw (A = 1): words [4][n / 4], the Philox block of each lane of four environments; n a multiple of 4
//     -> 0; 1 for a combination no family has; 2 where the header's two forms differ: scores, GREEDY and SAMPLE take the environments one by one (N = 1,
//        LunarLander's form) and, with n a multiple of 4, GREEDY and SAMPLE a second time four to a lane (N = 4, the classic kernels' form)
//   as a program (tests/test_mlp_policy_host.py): one-layer GREEDY cases on stdin, one per line, floats as 32-bit patterns in hex
//       "D A cont act H  <H (D + 1) + A (H + 1) policy words, nn.Linear order>  <D observation words>"
//     -> one line "action s_0 .. s_{A-1}" (hex words; cont = 1: the action word is the bits of s_0)
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../modurl_gym_amd/csrc/mlp2_policy.h"

using namespace mgym;

static bool same_action(bool is_float, uint32_t a, uint32_t b) { return a == b || (is_float && as_f32(a) != as_f32(a) && as_f32(b) != as_f32(b)); }

struct Case {
    int depth, head, H1, H2;
    const float* policy;
    float sigma;
    uint64_t n, stride;
    const float* obs;
    const uint32_t* words;
    uint32_t* actions;
    float* scores;
};

template <int D, int N>
static void gather(const Case& c, uint64_t first, float (&o)[N][D]) {
    for (int k = 0; k < N; ++k)
        for (int q = 0; q < D; ++q) o[k][q] = c.obs[(uint64_t)q * c.stride + first + k];
}

template <int D, int A, int ACT, int HEAD, class Net>
static int eval_head(const Net& net, const Case& c) {
    if constexpr ((HEAD == MLP_HEAD_GAUSS && A != 1) || (HEAD == MLP_HEAD_SAMPLE && A == 1)) return 1;
    else {
        const uint64_t n = c.n;
        if (HEAD == MLP_HEAD_GAUSS && n % 4) return 1;
        if constexpr (HEAD != MLP_HEAD_GAUSS)
            for (uint64_t i = 0; i < n; ++i) {
                float o[1][D];
                uint32_t a[1];
                gather<D, 1>(c, i, o);
                const uint32_t w[1] = {HEAD == MLP_HEAD_SAMPLE ? c.words[i] : 0u};
                mlp_actions<D, A, ACT, HEAD, 1>(net, o, w, c.sigma, a);
                c.actions[i] = a[0];
            }
        if (n % 4 == 0)
            for (uint64_t l = 0; l < n / 4; ++l) {
                float o[4][D];
                uint32_t w[4] = {0u, 0u, 0u, 0u}, a[4];
                gather<D, 4>(c, 4 * l, o);
                for (int k = 0; k < 4; ++k) {
                    if (HEAD == MLP_HEAD_SAMPLE) w[k] = c.words[4 * l + k];
                    if (HEAD == MLP_HEAD_GAUSS) w[k] = c.words[(uint64_t)k * (n / 4) + l];
                }
                mlp_actions<D, A, ACT, HEAD, 4>(net, o, w, c.sigma, a);
                for (int k = 0; k < 4; ++k) {
                    if (HEAD == MLP_HEAD_GAUSS) c.actions[4 * l + k] = a[k];
                    else if (!same_action(A == 1, c.actions[4 * l + k], a[k])) return 2;
                }
            }
        return 0;
    }
}

template <int D, int A, int ACT, class Net>
static int eval_net(const Net& net, const Case& c) {
    if (c.scores)
        for (uint64_t i = 0; i < c.n; ++i) {
            float o[1][D], s[1][A];
            gather<D, 1>(c, i, o);
            mlp_scores<D, A, ACT, 1>(net, o, s);
            for (int k = 0; k < A; ++k) c.scores[i * A + k] = s[0][k];
        }
    if (c.head == MLP_HEAD_GREEDY) return eval_head<D, A, ACT, MLP_HEAD_GREEDY>(net, c);
    if (c.head == MLP_HEAD_SAMPLE) return eval_head<D, A, ACT, MLP_HEAD_SAMPLE>(net, c);
    if (c.head == MLP_HEAD_GAUSS) return eval_head<D, A, ACT, MLP_HEAD_GAUSS>(net, c);
    return 1;
}

template <int D, int A, int ACT>
static int eval_depth(const Case& c) {
    if (c.H1 < 1 || c.H1 > kMlpMaxHidden) return 1;
    if (c.depth == 1) {
        MlpPack<D, A> p;
        mlp_pack<D, A>(c.policy, c.H1, p);
        return eval_net<D, A, ACT>(p, c);
    }
    if constexpr (ACT != MLP_ACT_TANH) {   // (no two-layer source has the exact tanh)
        if (c.depth == 2 && c.H2 >= 1 && c.H2 <= kMlpMaxHidden) {
            static float pack[kMlp2PackMax];   // (20 KB kept off the stack: policy_eval is not reentrant, and no test calls it from two threads)
            mlp2_pack(c.policy, D, A, c.H1, c.H2, pack);
            return eval_net<D, A, ACT>(Mlp2Net<D, A>{pack, c.H1, c.H2, c.sigma}, c);
        }
    }
    return 1;
}

template <int D, int A>
static int eval_act(int act, const Case& c) {
    if (act == MLP_ACT_RELU) return eval_depth<D, A, MLP_ACT_RELU>(c);
    if (act == MLP_ACT_TANH) return eval_depth<D, A, MLP_ACT_TANH>(c);
    if (act == MLP_ACT_TANH_FAST) return eval_depth<D, A, MLP_ACT_TANH_FAST>(c);
    return 1;
}

extern "C" int policy_eval(int D, int A, int depth, int act, int head, int H1, int H2, const float* policy, float sigma, uint64_t n, uint64_t stride,
                           const float* obs, const uint32_t* words, uint32_t* actions, float* scores) {
    const Case c{depth, head, H1, H2, policy, sigma, n, stride, obs, words, actions, scores};
    if (D == 4 && A == 2) return eval_act<4, 2>(act, c);   // CartPole
    if (D == 2 && A == 3) return eval_act<2, 3>(act, c);   // MountainCar
    if (D == 2 && A == 1) return eval_act<2, 1>(act, c);   // MountainCarContinuous
    if (D == 3 && A == 1) return eval_act<3, 1>(act, c);   // Pendulum
    if (D == 6 && A == 3) return eval_act<6, 3>(act, c);   // Acrobot
    if (D == 8 && A == 4) return eval_act<8, 4>(act, c);   // LunarLander
    return 1;
}

static bool rd(float& f) {
    unsigned long long u;
    if (scanf("%llx", &u) != 1) return false;
    const uint32_t w = (uint32_t)u;
    memcpy(&f, &w, 4);
    return true;
}

int main() {
    int D, A, cont, act, H;
    while (scanf("%d %d %d %d %d", &D, &A, &cont, &act, &H) == 5) {
        if (D < 1 || D > 8 || A < 1 || A > 4 || H < 1 || H > kMlpMaxHidden || (cont != 0) != (A == 1)) return 2;
        std::vector<float> pol(mlp_policy_floats(D, A, H));
        float o[8], s[4];
        uint32_t a;
        for (float& v : pol) if (!rd(v)) return 2;
        for (int q = 0; q < D; ++q) if (!rd(o[q])) return 2;
        if (policy_eval(D, A, 1, act, MLP_HEAD_GREEDY, H, 0, pol.data(), 0.0f, 1, 1, o, nullptr, &a, s)) return 2;
        printf("%x", a);
        for (int k = 0; k < A; ++k) { uint32_t w; memcpy(&w, &s[k], 4); printf(" %x", w); }
        printf("\n");
    }
    return 0;
}
