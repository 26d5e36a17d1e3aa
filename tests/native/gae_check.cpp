// CPU check of the advantage / episode-return scans (modurl_gym_amd/csrc/gae.h: the lines the kernels of gae.hip compile), built as a shared object with
// g++ -ffp-contract=off for tests/test_gae_host.py and the GPU tests.
//   gae_eval(K, n, reward, done, trunc, value, last_value, final_value, gamma, lambda, adv_out, ret_out) -> 0: gae_env over every environment; gl is the one
//     f32 product gamma * lambda, as mgym_gae forms it on the host.  done / trunc / final_value and either output may be NULL.
//   ep_eval(K, n, reward, done, trunc, ep_return, ep_length, return_out, length_out) -> 0: ep_env over every environment
//   gae_batch() -> kGaeBatch
#include <stdint.h>
#include "../../modurl_gym_amd/csrc/gae.h"

using namespace mgym;

extern "C" {

int gae_eval(int32_t K, uint64_t n, const float* reward, const uint8_t* done, const uint8_t* trunc, const float* value, const float* last_value,
             const float* final_value, float gamma, float lambda, float* adv_out, float* ret_out) {
    const float gl = gamma * lambda;
    for (uint64_t i = 0; i < n; ++i) gae_env(K, n, i, reward, done, trunc, value, last_value, final_value, gamma, gl, adv_out, ret_out);
    return 0;
}

int ep_eval(int32_t K, uint64_t n, const float* reward, const uint8_t* done, const uint8_t* trunc, float* ep_return, uint32_t* ep_length, float* return_out,
            uint32_t* length_out) {
    for (uint64_t i = 0; i < n; ++i) ep_env(K, n, i, reward, done, trunc, ep_return, ep_length, return_out, length_out);
    return 0;
}

int gae_batch(void) { return kGaeBatch; }

}
