// policy.h — where a fused rollout takes its actions from: the one description every family's kernels and host wrappers share.
#pragma once
#include <stdint.h>

namespace mgym {

// The action source of a rollout launch (a template parameter of the families' rollout kernels):
//   TABLE     the caller's [K][n] actions (mgym_rollout)
//   LINEAR    one score per action from the observation the env holds before the step (mgym_rollout_linear)
//   UNIFORM   Philox draws keyed by (policy seed, global env id, number of earlier uniform calls on the handle, step) (mgym_rollout_uniform)
//   MLP_RELU / MLP_TANH  as LINEAR, decided by mlp_policy.h's one-hidden-layer policy (mgym_rollout_mlp)
// How LunarLander's persistent launch carries each of them: ll_roll_types.h.
enum { ROLL_ACT_TABLE = 0, ROLL_ACT_LINEAR = 1, ROLL_ACT_UNIFORM = 2, ROLL_ACT_MLP_RELU = 3, ROLL_ACT_MLP_TANH = 4 };
// the hidden-layer sources
constexpr bool roll_act_is_mlp(int source) { return source == ROLL_ACT_MLP_RELU || source == ROLL_ACT_MLP_TANH; }
// the sources that decide from the observation
constexpr bool roll_act_observes(int source) { return source == ROLL_ACT_LINEAR || roll_act_is_mlp(source); }

// One call of mgym_rollout_uniform / _linear / _mlp as the C ABI hands it to Env::rollout_policy, its own argument checks passed.
struct PolicyCall {
    int source;             // ROLL_ACT_UNIFORM, ROLL_ACT_LINEAR, ROLL_ACT_MLP_RELU or ROLL_ACT_MLP_TANH
    const char* api;        // the entry point's name: the prefix of every error message
    const float* weights;   // LINEAR: obs_dim weights + bias per score; MLP_*: W1[H][D], b1[H], W2[A][H], b2[A] (host floats); UNIFORM: null
    int hidden;             // MLP_*: H
    uint64_t seed;          // UNIFORM: the policy seed
};

}  // namespace mgym
