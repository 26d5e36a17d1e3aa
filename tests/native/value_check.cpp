// CPU check of mgym_value_mlp's mapping (modurl_gym_amd/csrc/value.h over mlp_policy.h and mlp2_policy.h: the lines the kernels of value.hip compile), built as
// a shared object with g++ -ffp-contract=off for tests/value_ref.py.
//   value_eval(D, depth, act, H1, H2, critic, K, n, obs_first, obs, final_obs, done, trunc, value_out, last_value_out, final_value_out)
//     depth 1 (critic: W1[H1][D], b1, W2[1][H1], b2; H2 is ignored) or 2 (W1[H1][D], b1, W2[H2][H1], b2, W3[1][H2], b3; no MLP_ACT_TANH): value_env over every
//     environment.  final_obs / trunc / final_value_out all NULL or all set; done may be NULL.
//     -> 0; 1 for a combination the entry point refuses; 2 where, with n a multiple of 4, the dense rows taken four to a lane (mlp_scores<D, 1, ACT, 4>, the
//        form of learner.h's dense4_kernel) differ from value_env's
//   value_chunk() -> kValueChunk;  value_wave_envs() -> kValueWaveEnvs
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../modurl_gym_amd/csrc/value.h"

using namespace mgym;

struct Case {
    int32_t K;
    uint64_t n;
    const float *obs_first, *obs, *final_obs;
    const uint8_t *done, *trunc;
    float *value_out, *last_value_out, *final_value_out;
};

template <int D, int ACT, class Net>
static int eval(const Net& net, const Case& c) {
    for (uint64_t i = 0; i < c.n; ++i) value_env<D, ACT>(net, c.K, c.n, i, c.obs_first, c.obs, c.final_obs, c.done, c.trunc, c.value_out, c.last_value_out, c.final_value_out);
    if (c.n % 4) return 0;
    for (int32_t r = 0; r <= c.K; ++r) {
        const float* in = value_row_in(r, c.n, D, c.obs_first, c.obs);
        const float* out = value_row_out(r, c.K, c.n, c.value_out, c.last_value_out);
        for (uint64_t l = 0; l < c.n / 4; ++l) {
            float o[4][D], s[4][1];
            for (int k = 0; k < 4; ++k)
                for (int q = 0; q < D; ++q) o[k][q] = in[(uint64_t)q * c.n + 4 * l + k];
            mlp_scores<D, 1, ACT, 4>(net, o, s);
            for (int k = 0; k < 4; ++k) {
                const uint32_t a = as_u32(s[k][0]), b = as_u32(out[4 * l + k]);
                if (a != b && !(s[k][0] != s[k][0] && out[4 * l + k] != out[4 * l + k])) return 2;
            }
        }
    }
    return 0;
}

template <int D>
static int eval_dim(int depth, int act, int H1, int H2, const float* critic, const Case& c) {
    if (depth == 1) {
        MlpPack<D, 1> pack;
        mlp_pack<D, 1>(critic, H1, pack);
        if (act == MLP_ACT_RELU) return eval<D, MLP_ACT_RELU>(pack, c);
        if (act == MLP_ACT_TANH) return eval<D, MLP_ACT_TANH>(pack, c);
        if (act == MLP_ACT_TANH_FAST) return eval<D, MLP_ACT_TANH_FAST>(pack, c);
        return 1;
    }
    std::vector<float> pack(mlp2_pack_floats(D, H1, H2));
    mlp2_pack(critic, D, 1, H1, H2, pack.data());
    const Mlp2Net<D, 1> net{pack.data(), H1, H2, 0.0f};
    if (act == MLP_ACT_RELU) return eval<D, MLP_ACT_RELU>(net, c);
    if (act == MLP_ACT_TANH_FAST) return eval<D, MLP_ACT_TANH_FAST>(net, c);
    return 1;
}

extern "C" {

int value_eval(int D, int depth, int act, int H1, int H2, const float* critic, int32_t K, uint64_t n, const float* obs_first, const float* obs, const float* final_obs,
               const uint8_t* done, const uint8_t* trunc, float* value_out, float* last_value_out, float* final_value_out) {
    if (H1 < 1 || H1 > kMlpMaxHidden || (depth == 2 && (H2 < 1 || H2 > kMlpMaxHidden)) || (depth != 1 && depth != 2) || K < 1) return 1;
    if ((final_obs != nullptr) != (final_value_out != nullptr) || (final_obs && !trunc)) return 1;
    const Case c{K, n, obs_first, obs, final_obs, done, trunc, value_out, last_value_out, final_value_out};
    switch (D) {
    case 2: return eval_dim<2>(depth, act, H1, H2, critic, c);
    case 3: return eval_dim<3>(depth, act, H1, H2, critic, c);
    case 4: return eval_dim<4>(depth, act, H1, H2, critic, c);
    case 6: return eval_dim<6>(depth, act, H1, H2, critic, c);
    case 8: return eval_dim<8>(depth, act, H1, H2, critic, c);
    }
    return 1;
}

int value_chunk(void) { return kValueChunk; }
int value_wave_envs(void) { return kValueWaveEnvs; }

}
