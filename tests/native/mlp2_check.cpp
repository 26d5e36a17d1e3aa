// CPU check of the two-hidden-layer policy header (modurl_gym_amd/csrc/mlp2_policy.h: the lines the rollout kernels compile), built as a shared object with
// g++ -ffp-contract=off for tests/test_mlp2_host.py and tests/test_gpu_mlp2.py.
//   mlp2_eval(D, A, act, head, H1, H2, policy, sigma, n, obs [D][n], words, actions [n], scores [n][A] or NULL) -> 0, or 1 for a combination no family has
//     head 0  the argmax (A > 1) or the bits of the one score (A = 1)
//     head 1  the categorical draw (A > 1): words [n], one Philox word per environment
//     head 2  the Gaussian draw (A = 1): words [4][n / 4], the Philox block of each lane of four environments; n a multiple of 4
//   Scores and the heads 0 and 1 take the environments one by one (N = 1, LunarLander's form); with n a multiple of 4 they are evaluated a second time four to a
//   lane (N = 4, the classic kernels' packed pairs) and a difference between the two forms is status 2.
//   mlp2_one_layer_scores(D, A, H, policy, n, obs, scores [n][A]): mlp_policy.h's one-hidden-layer ReLU scores, for the identity-middle-layer check
#include <stdint.h>
#include <string.h>
#include "../../modurl_gym_amd/csrc/mlp2_policy.h"

using namespace mgym;

template <int D, int A, int ACT, int HEAD>
static int eval_head(const Mlp2Net<D, A>& net, float sigma, uint64_t n, const float* obs, const uint32_t* words, uint32_t* actions) {
    if constexpr (HEAD == MLP2_HEAD_GAUSS && A != 1) return 1;
    else if constexpr (HEAD == MLP2_HEAD_SAMPLE && A == 1) return 1;
    else {
        if (HEAD == MLP2_HEAD_GAUSS && n % 4) return 1;
        if constexpr (HEAD != MLP2_HEAD_GAUSS)
            for (uint64_t i = 0; i < n; ++i) {
                float o[1][D];
                uint32_t a[1];
                for (int q = 0; q < D; ++q) o[0][q] = obs[(uint64_t)q * n + i];
                const uint32_t w[1] = {HEAD == MLP2_HEAD_SAMPLE ? words[i] : 0u};
                mlp2_actions<D, A, ACT, HEAD, 1>(net, o, w, sigma, a);
                actions[i] = a[0];
            }
        if (n % 4 == 0)
            for (uint64_t l = 0; l < n / 4; ++l) {
                float o[4][D];
                uint32_t w[4] = {0u, 0u, 0u, 0u}, a[4];
                for (int k = 0; k < 4; ++k) {
                    for (int q = 0; q < D; ++q) o[k][q] = obs[(uint64_t)q * n + 4 * l + k];
                    if (HEAD == MLP2_HEAD_SAMPLE) w[k] = words[4 * l + k];
                    if (HEAD == MLP2_HEAD_GAUSS) w[k] = words[(uint64_t)k * (n / 4) + l];
                }
                mlp2_actions<D, A, ACT, HEAD, 4>(net, o, w, sigma, a);
                for (int k = 0; k < 4; ++k) {
                    if (HEAD == MLP2_HEAD_GAUSS) actions[4 * l + k] = a[k];
                    else if (actions[4 * l + k] != a[k] && !(A == 1 && as_f32(a[k]) != as_f32(a[k]) && as_f32(actions[4 * l + k]) != as_f32(actions[4 * l + k]))) return 2;
                }
            }
        return 0;
    }
}

template <int D, int A, int ACT>
static int eval_act(int head, int H1, int H2, const float* policy, float sigma, uint64_t n, const float* obs, const uint32_t* words, uint32_t* actions, float* scores) {
    static float pack[kMlp2PackMax];
    mlp2_pack(policy, D, A, H1, H2, pack);
    const Mlp2Net<D, A> net{pack, H1, H2, sigma};
    if (scores)
        for (uint64_t i = 0; i < n; ++i) {
            float o[1][D], s[1][A];
            for (int q = 0; q < D; ++q) o[0][q] = obs[(uint64_t)q * n + i];
            mlp2_scores<D, A, ACT, 1>(net, o, s);
            for (int k = 0; k < A; ++k) scores[i * A + k] = s[0][k];
        }
    if (head == MLP2_HEAD_GREEDY) return eval_head<D, A, ACT, MLP2_HEAD_GREEDY>(net, sigma, n, obs, words, actions);
    if (head == MLP2_HEAD_SAMPLE) return eval_head<D, A, ACT, MLP2_HEAD_SAMPLE>(net, sigma, n, obs, words, actions);
    return eval_head<D, A, ACT, MLP2_HEAD_GAUSS>(net, sigma, n, obs, words, actions);
}

template <int D, int A>
static int eval(int act, int head, int H1, int H2, const float* policy, float sigma, uint64_t n, const float* obs, const uint32_t* words, uint32_t* actions, float* scores) {
    if (act == MLP_ACT_RELU) return eval_act<D, A, MLP_ACT_RELU>(head, H1, H2, policy, sigma, n, obs, words, actions, scores);
    return eval_act<D, A, MLP_ACT_TANH_FAST>(head, H1, H2, policy, sigma, n, obs, words, actions, scores);
}

extern "C" int mlp2_eval(int D, int A, int act, int head, int H1, int H2, const float* policy, float sigma, uint64_t n, const float* obs, const uint32_t* words,
                         uint32_t* actions, float* scores) {
    if (H1 < 1 || H1 > kMlpMaxHidden || H2 < 1 || H2 > kMlpMaxHidden || head < 0 || head > 2 || (act != MLP_ACT_RELU && act != MLP_ACT_TANH_FAST)) return 1;
    if (D == 4 && A == 2) return eval<4, 2>(act, head, H1, H2, policy, sigma, n, obs, words, actions, scores);   // CartPole
    if (D == 2 && A == 3) return eval<2, 3>(act, head, H1, H2, policy, sigma, n, obs, words, actions, scores);   // MountainCar
    if (D == 2 && A == 1) return eval<2, 1>(act, head, H1, H2, policy, sigma, n, obs, words, actions, scores);   // MountainCarContinuous
    if (D == 3 && A == 1) return eval<3, 1>(act, head, H1, H2, policy, sigma, n, obs, words, actions, scores);   // Pendulum
    if (D == 6 && A == 3) return eval<6, 3>(act, head, H1, H2, policy, sigma, n, obs, words, actions, scores);   // Acrobot
    if (D == 8 && A == 4) return eval<8, 4>(act, head, H1, H2, policy, sigma, n, obs, words, actions, scores);   // LunarLander
    return 1;
}

template <int D, int A>
static int one_layer(int H, const float* policy, uint64_t n, const float* obs, float* scores) {
    MlpPack<D, A> p;
    mlp_pack<D, A>(policy, H, p);
    for (uint64_t i = 0; i < n; ++i) {
        float o[1][D], s[1][A];
        for (int q = 0; q < D; ++q) o[0][q] = obs[(uint64_t)q * n + i];
        mlp_scores<D, A, MLP_ACT_RELU, 1>(p, o, s);
        for (int k = 0; k < A; ++k) scores[i * A + k] = s[0][k];
    }
    return 0;
}

extern "C" int mlp2_one_layer_scores(int D, int A, int H, const float* policy, uint64_t n, const float* obs, float* scores) {
    if (H < 1 || H > kMlpMaxHidden) return 1;
    if (D == 4 && A == 2) return one_layer<4, 2>(H, policy, n, obs, scores);
    if (D == 2 && A == 3) return one_layer<2, 3>(H, policy, n, obs, scores);
    if (D == 2 && A == 1) return one_layer<2, 1>(H, policy, n, obs, scores);
    if (D == 3 && A == 1) return one_layer<3, 1>(H, policy, n, obs, scores);
    if (D == 6 && A == 3) return one_layer<6, 3>(H, policy, n, obs, scores);
    if (D == 8 && A == 4) return one_layer<8, 4>(H, policy, n, obs, scores);
    return 1;
}
