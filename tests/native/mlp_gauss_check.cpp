// CPU check of the draw of mgym_rollout_mlp_gauss (mg_log_u25 and mlp_gauss_pair in modurl_gym_amd/csrc/mlp_policy.h, the lines the kernels compile), built
// with g++ -ffp-contract=off as a shared object (tests/mlp_gauss_ref.py):
//   mlp_gauss_eval      one pair of Philox words per case -> z_even, z_odd, q and (if asked) the f64 logarithm L
// The GAUSS head of mlp_actions, which calls these, is checked by tests/native/policy_check.cpp.
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
