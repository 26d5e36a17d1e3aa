// CPU check of the draw of mgym_rollout_mlp_gauss (mg_log_u25, mlp_gauss_pair and the GAUSS form of mlp_actions in modurl_gym_amd/csrc/mlp_policy.h, the
// lines the kernels compile), built with g++ -ffp-contract=off as a shared object (tests/mlp_gauss_ref.py):
//   mlp_gauss_eval      one pair of Philox words per case -> z_even, z_odd, q and (if asked) the f64 logarithm L
//   mlp_gauss_actions   the lane form: four environments per Philox block -> the action words mu + sigma * z under a hidden-layer policy
#include <stdint.h>
#include "../../modurl_gym_amd/csrc/mlp_policy.h"

using namespace mgym;

// wa, wb, z_even, z_odd: [n]; q: [n] floats or NULL; L: [n] doubles or NULL
extern "C" void mlp_gauss_eval(uint64_t n, const uint32_t* wa, const uint32_t* wb, float* z_even, float* z_odd, float* q, double* L) {
    for (uint64_t i = 0; i < n; ++i) {
        mlp_gauss_pair(wa[i], wb[i], &z_even[i], &z_odd[i]);
        if (q) q[i] = mlp_gauss_q(wa[i]);
        if (L) L[i] = mg_log_u25(2u * (wa[i] >> 8) + 1u);
    }
}

template <int D, int ACT>
static void actions(const float* policy, int H, float sigma, uint64_t n, const float* obs, const uint32_t* words, uint32_t* act) {
    MlpPack<D, 1> pack;
    mlp_pack<D, 1>(policy, H, pack);
    for (uint64_t i0 = 0; i0 < n; i0 += 4) {
        float o[4][D];
        uint32_t w[4], a[4];
        for (int k = 0; k < 4; ++k) {
            for (int q = 0; q < D; ++q) o[k][q] = obs[(uint64_t)q * n + i0 + k];
            w[k] = words[(uint64_t)k * (n / 4) + i0 / 4];
        }
        mlp_actions<D, ACT>(pack, o, w, sigma, a);
        for (int k = 0; k < 4; ++k) act[i0 + k] = a[k];
    }
}

// policy: H (D + 1) + (H + 1) floats in nn.Linear order; obs: [D][n]; words: [4][n / 4], the four words of each lane's Philox block; act: [n] action words.
// Returns 0, or 1 for a D other than 2 or 3, an activation other than 0 / 1, an H outside 1 .. 64 or an n that is no multiple of 4.
extern "C" int mlp_gauss_actions(int D, int activation, int H, const float* policy, float sigma, uint64_t n, const float* obs, const uint32_t* words, uint32_t* act) {
    if (H < 1 || H > kMlpMaxHidden || n % 4 != 0) return 1;
    if (D == 2 && activation == MLP_ACT_RELU) actions<2, MLP_ACT_RELU>(policy, H, sigma, n, obs, words, act);
    else if (D == 2 && activation == MLP_ACT_TANH) actions<2, MLP_ACT_TANH>(policy, H, sigma, n, obs, words, act);
    else if (D == 3 && activation == MLP_ACT_RELU) actions<3, MLP_ACT_RELU>(policy, H, sigma, n, obs, words, act);
    else if (D == 3 && activation == MLP_ACT_TANH) actions<3, MLP_ACT_TANH>(policy, H, sigma, n, obs, words, act);
    else return 1;
    return 0;
}
