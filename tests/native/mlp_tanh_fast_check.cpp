// CPU check of the MLP policy header with the MGYM_ACT_TANH_FAST activation (modurl_gym_amd/csrc/mlp_policy.h, ACT = MLP_ACT_TANH_FAST: the lines the
// rollout kernels compile), built as a shared object with g++ -ffp-contract=off for tests/test_mlp_tanh_fast_host.py and tests/test_gpu_mlp_tanh_fast.py.
//   mlp_tanh_fast_eval(D, A, form, H, policy, sigma, n, obs [D][n], words, actions [n], scores [n][A] or NULL) -> 0, or 1 for a combination no family has
//     form 0  the argmax (A > 1) or the bits of the one score (A = 1)
//     form 1  the categorical draw (A > 1): words [n], one Philox word per environment
//     form 2  the Gaussian draw (A = 1): words [4][n / 4], the Philox block of each lane of four environments; n a multiple of 4
#include <stdint.h>
#include "../../modurl_gym_amd/csrc/mlp_policy.h"

using namespace mgym;

template <int D, int A>
static int eval(int form, int H, const float* policy, float sigma, uint64_t n, const float* obs, const uint32_t* words, uint32_t* actions, float* scores) {
    constexpr int ACT = MLP_ACT_TANH_FAST;
    MlpPack<D, A> p;
    mlp_pack<D, A>(policy, H, p);
    if (scores)
        for (uint64_t i = 0; i < n; ++i) {
            float o[1][D], s[1][A];
            for (int q = 0; q < D; ++q) o[0][q] = obs[(uint64_t)q * n + i];
            mlp_scores<D, A, ACT, 1>(p, o, s);
            for (int k = 0; k < A; ++k) scores[i * A + k] = s[0][k];
        }
    if (form == 2) {
        if constexpr (A == 1) {
            if (n % 4) return 1;
            for (uint64_t l = 0; l < n / 4; ++l) {
                float o[4][D];
                uint32_t w[4], a[4];
                for (int k = 0; k < 4; ++k) {
                    for (int q = 0; q < D; ++q) o[k][q] = obs[(uint64_t)q * n + 4 * l + k];
                    w[k] = words[(uint64_t)k * (n / 4) + l];
                }
                mlp_actions<D, ACT>(p, o, w, sigma, a);
                for (int k = 0; k < 4; ++k) actions[4 * l + k] = a[k];
            }
            return 0;
        }
        return 1;
    }
    for (uint64_t i = 0; i < n; ++i) {
        float o[1][D];
        uint32_t a[1];
        for (int q = 0; q < D; ++q) o[0][q] = obs[(uint64_t)q * n + i];
        if (form == 0) {
            mlp_actions<D, A, ACT, A == 1, 1>(p, o, a);
        } else {
            if constexpr (A > 1) {
                const uint32_t w[1] = {words[i]};
                mlp_actions<D, A, ACT, 1>(p, o, w, a);
            } else {
                return 1;
            }
        }
        actions[i] = a[0];
    }
    return 0;
}

extern "C" int mlp_tanh_fast_eval(int D, int A, int form, int H, const float* policy, float sigma, uint64_t n, const float* obs, const uint32_t* words,
                                  uint32_t* actions, float* scores) {
    if (H < 1 || H > kMlpMaxHidden || form < 0 || form > 2) return 1;
    if (D == 4 && A == 2) return eval<4, 2>(form, H, policy, sigma, n, obs, words, actions, scores);   // CartPole
    if (D == 2 && A == 3) return eval<2, 3>(form, H, policy, sigma, n, obs, words, actions, scores);   // MountainCar
    if (D == 2 && A == 1) return eval<2, 1>(form, H, policy, sigma, n, obs, words, actions, scores);   // MountainCarContinuous
    if (D == 3 && A == 1) return eval<3, 1>(form, H, policy, sigma, n, obs, words, actions, scores);   // Pendulum
    if (D == 6 && A == 3) return eval<6, 3>(form, H, policy, sigma, n, obs, words, actions, scores);   // Acrobot
    if (D == 8 && A == 4) return eval<8, 4>(form, H, policy, sigma, n, obs, words, actions, scores);   // LunarLander
    return 1;
}
