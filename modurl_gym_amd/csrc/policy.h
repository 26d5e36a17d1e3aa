// policy.h — where a fused rollout takes its actions from: the one description every family's kernels and host wrappers share.
#pragma once
#include <stdint.h>
#include <type_traits>
#include "mlp_policy.h"
#include "mlp2_policy.h"
#include "philox.h"

namespace mgym {

// The action source of a rollout launch (a template parameter of the families' rollout kernels):
//   TABLE     the caller's [K][n] actions (mgym_rollout)
//   LINEAR    one score per action from the observation the env holds before the step (mgym_rollout_linear)
//   UNIFORM   Philox draws keyed by (policy seed, global env id, number of earlier uniform calls on the handle, step) (mgym_rollout_uniform)
//   MLP_RELU / MLP_TANH  as LINEAR, decided by mlp_policy.h's one-hidden-layer policy (mgym_rollout_mlp)
//   MLP_RELU_SAMPLE / MLP_TANH_SAMPLE  the same scores, the action drawn from their softmax with a Philox word keyed by (policy seed, global env id, the
//             caller's call word, step) (mgym_rollout_mlp_sample).  New sources, not a flag: the instantiations of the others keep their code.
//   MLP_RELU_GAUSS / MLP_TANH_GAUSS  the continuous families' one score as the mean of a Gaussian: the action is mu + sigma * z, z a Box-Muller normal from a
//             Philox block keyed the same way (mgym_rollout_mlp_gauss).  New sources again, for the same reason.
//   MLP_TANH_FAST / MLP_TANH_FAST_SAMPLE / MLP_TANH_FAST_GAUSS  the three forms above with mg_tanhf_fast as the hidden activation (MGYM_ACT_TANH_FAST).  New
//             sources once more: the nine before them keep their numbers and their code.  LunarLander's persistent launch carries none of them.
//   MLP2_*    the two-hidden-layer policy of mlp2_policy.h (mgym_rollout_mlp2): 12 + 2 * head + (1 for MGYM_ACT_TANH_FAST), head = MGYM_HEAD_GREEDY / _SAMPLE /
//             _GAUSS.  New sources beside the twelve, which keep their numbers and their code; their weights are the handle's pack in device memory, not a
//             kernel argument.  LunarLander's persistent launch carries none of them.
// How LunarLander's persistent launch carries each of them: ll_roll_types.h.
enum { ROLL_ACT_TABLE = 0, ROLL_ACT_LINEAR = 1, ROLL_ACT_UNIFORM = 2, ROLL_ACT_MLP_RELU = 3, ROLL_ACT_MLP_TANH = 4, ROLL_ACT_MLP_RELU_SAMPLE = 5,
       ROLL_ACT_MLP_TANH_SAMPLE = 6, ROLL_ACT_MLP_RELU_GAUSS = 7, ROLL_ACT_MLP_TANH_GAUSS = 8, ROLL_ACT_MLP_TANH_FAST = 9, ROLL_ACT_MLP_TANH_FAST_SAMPLE = 10,
       ROLL_ACT_MLP_TANH_FAST_GAUSS = 11, ROLL_ACT_MLP2_RELU = 12, ROLL_ACT_MLP2_TANH_FAST = 13, ROLL_ACT_MLP2_RELU_SAMPLE = 14, ROLL_ACT_MLP2_TANH_FAST_SAMPLE = 15,
       ROLL_ACT_MLP2_RELU_GAUSS = 16, ROLL_ACT_MLP2_TANH_FAST_GAUSS = 17 };
// the hidden-layer sources that draw their action from the categorical distribution (LunarLander's persistent launch carries none of them)
constexpr bool roll_act_samples(int source) { return source == ROLL_ACT_MLP_RELU_SAMPLE || source == ROLL_ACT_MLP_TANH_SAMPLE || source == ROLL_ACT_MLP_TANH_FAST_SAMPLE; }
// the hidden-layer sources that draw a continuous action around their score (MountainCarContinuous and Pendulum only)
constexpr bool roll_act_gauss(int source) { return source == ROLL_ACT_MLP_RELU_GAUSS || source == ROLL_ACT_MLP_TANH_GAUSS || source == ROLL_ACT_MLP_TANH_FAST_GAUSS; }
// the hidden-layer sources
constexpr bool roll_act_is_mlp(int source) {
    return source == ROLL_ACT_MLP_RELU || source == ROLL_ACT_MLP_TANH || source == ROLL_ACT_MLP_TANH_FAST || roll_act_samples(source) || roll_act_gauss(source);
}
// and back from an activation (MLP_ACT_*) and a head to the source: the one-layer sources by head, the two-layer ones as 12 + 2 * head + (1 for TANH_FAST)
constexpr int roll_act_mlp_plain(int act) { return act == MLP_ACT_TANH_FAST ? ROLL_ACT_MLP_TANH_FAST : act == MLP_ACT_TANH ? ROLL_ACT_MLP_TANH : ROLL_ACT_MLP_RELU; }
constexpr int roll_act_mlp_sample(int act) { return act == MLP_ACT_TANH_FAST ? ROLL_ACT_MLP_TANH_FAST_SAMPLE : act == MLP_ACT_TANH ? ROLL_ACT_MLP_TANH_SAMPLE : ROLL_ACT_MLP_RELU_SAMPLE; }
constexpr int roll_act_mlp_gauss(int act) { return act == MLP_ACT_TANH_FAST ? ROLL_ACT_MLP_TANH_FAST_GAUSS : act == MLP_ACT_TANH ? ROLL_ACT_MLP_TANH_GAUSS : ROLL_ACT_MLP_RELU_GAUSS; }
constexpr bool roll_act_is_mlp2(int source) { return source >= ROLL_ACT_MLP2_RELU && source <= ROLL_ACT_MLP2_TANH_FAST_GAUSS; }
constexpr int roll_act_mlp2(int act, int head) { return ROLL_ACT_MLP2_RELU + 2 * head + (act == MLP_ACT_TANH_FAST ? 1 : 0); }
// The one mapping from a hidden-layer source of either depth to the call that decides its action, read by the kernels and the host wrappers alike: the
// head (MLP_HEAD_*; -1 for any other source), the hidden activation (MLP_ACT_*), and the Philox slot a drawing head counts its steps from
constexpr int roll_act_head(int source) {
    return roll_act_is_mlp2(source) ? (source - ROLL_ACT_MLP2_RELU) / 2
           : roll_act_samples(source) ? MLP_HEAD_SAMPLE : roll_act_gauss(source) ? MLP_HEAD_GAUSS : roll_act_is_mlp(source) ? MLP_HEAD_GREEDY : -1;
}
constexpr int roll_act_hidden_act(int source) {
    return roll_act_is_mlp2(source) ? (((source - ROLL_ACT_MLP2_RELU) & 1) ? MLP_ACT_TANH_FAST : MLP_ACT_RELU)
           : source == ROLL_ACT_MLP_TANH || source == ROLL_ACT_MLP_TANH_SAMPLE || source == ROLL_ACT_MLP_TANH_GAUSS ? MLP_ACT_TANH
           : source == ROLL_ACT_MLP_TANH_FAST || source == ROLL_ACT_MLP_TANH_FAST_SAMPLE || source == ROLL_ACT_MLP_TANH_FAST_GAUSS ? MLP_ACT_TANH_FAST
                                                                                                                                  : MLP_ACT_RELU;
}
constexpr uint32_t policy_head_slot(int head) { return head == MLP_HEAD_GAUSS ? SLOT_POLICY_GAUSS : SLOT_POLICY_SAMPLE; }
// the policy sources a family with discrete actions has kernels for (all but the Gaussian draws), and one with a continuous action (all but the categorical)
constexpr bool roll_act_discrete_takes(int source) { return roll_act_head(source) != MLP_HEAD_GAUSS; }
constexpr bool roll_act_box_takes(int source) { return roll_act_head(source) != MLP_HEAD_SAMPLE; }
// every source, walked once at compile time: the two mappings against the ways back
template <int S = ROLL_ACT_TABLE>
constexpr bool roll_act_mappings_agree() {
    constexpr int head = roll_act_head(S), act = roll_act_hidden_act(S);
    constexpr int back = head == MLP_HEAD_GREEDY ? roll_act_mlp_plain(act) : head == MLP_HEAD_SAMPLE ? roll_act_mlp_sample(act) : roll_act_mlp_gauss(act);
    static_assert((head >= 0) == (roll_act_is_mlp(S) || roll_act_is_mlp2(S)), "the hidden-layer sources, and only they, have a head");
    static_assert(!roll_act_is_mlp(S) || back == S, "a one-layer source is the plain / _sample / _gauss source of its activation");
    static_assert(!roll_act_is_mlp2(S) || roll_act_mlp2(act, head) == S, "a two-layer source is roll_act_mlp2 of its activation and head");
    static_assert(roll_act_discrete_takes(S) || roll_act_box_takes(S), "every source has a family");
    if constexpr (S < ROLL_ACT_MLP2_TANH_FAST_GAUSS) return roll_act_mappings_agree<S + 1>();
    else return true;
}
static_assert(roll_act_mappings_agree(), "all seventeen sources and the table");
// from the run-time source of a PolicyCall to the source as a template argument, as with_bools (common.h) does for bools: f(std::integral_constant<int, ROLL_ACT_*>{})
// for the one of ROLL_ACT_LINEAR .. ROLL_ACT_MLP2_TANH_FAST_GAUSS that `source` is (the table is no policy call)
template <int S = ROLL_ACT_LINEAR, class F>
void with_policy_source(F&& f, int source) {
    if (source == S) f(std::integral_constant<int, S>{});
    else if constexpr (S < ROLL_ACT_MLP2_TANH_FAST_GAUSS) with_policy_source<S + 1>(f, source);
}
// the sources that decide from the observation
constexpr bool roll_act_observes(int source) { return source == ROLL_ACT_LINEAR || roll_act_is_mlp(source); }

// One call of mgym_rollout_uniform / _linear / _mlp / _mlp_sample / _mlp_gauss / _mlp2 as the C ABI hands it to Env::rollout_policy, its own argument checks passed.
struct PolicyCall {
    int source;             // ROLL_ACT_UNIFORM, ROLL_ACT_LINEAR or one of the ROLL_ACT_MLP_* / ROLL_ACT_MLP2_* sources
    const char* api;        // the entry point's name: the prefix of every error message
    const float* weights;   // LINEAR: obs_dim weights + bias per score; MLP_*: W1[H][D], b1[H], W2[A][H], b2[A] (host floats); UNIFORM: null
    int hidden;             // MLP_*: H
    uint64_t seed;          // UNIFORM, MLP_*_SAMPLE, MLP_*_GAUSS: the policy seed
    uint32_t call;          // MLP_*_SAMPLE, MLP_*_GAUSS: the caller's call word (UNIFORM counts its calls on the handle instead)
    float sigma;            // MLP_*_GAUSS: the standard deviation, finite and >= 0
    int hidden2 = 0;        // MLP2_*: H2 (`hidden` is H1, `weights` W1[H1][D], b1[H1], W2[H2][H1], b2[H2], W3[A][H2], b3[A])
};

// the uniform stream of a classic family's rollout kernel (policy seed, call word); the categorical draw of MLP_*_SAMPLE travels in it too
struct UniformDraw { uint64_t seed; uint32_t call; };
// what a Gaussian-drawing hidden-layer source takes in its place
struct GaussDraw { uint64_t seed; uint32_t call; float sigma; };

// What a classic family's rollout kernel takes for POLICY: the weight pack of mlp_policy.h in the place of the family's linear words (the one-layer sources;
// the two-layer ones take their Mlp2Net at the head of the trailing pack, soa4.h), and the draw.  Aliases: they do not enter the kernels' mangled names.
template <int POLICY, int D, int A, class Linear> using PolicyArg = std::conditional_t<roll_act_is_mlp(POLICY), MlpPack<D, A>, Linear>;
template <int POLICY> using DrawArg = std::conditional_t<roll_act_gauss(POLICY), GaussDraw, UniformDraw>;

// ---- the hidden-layer sources of both depths in a classic rollout kernel, for a lane of four (global ids g .. g + 3, g a multiple of 4) at step t ----
// the sigma of a kernel's DrawArg (a two-layer source's is in its Mlp2Net), and the Mlp2Net at the head of a kernel's trailing pack (soa4.h)
__device__ __forceinline__ float draw_sigma(const UniformDraw&) { return 0.0f; }
__device__ __forceinline__ float draw_sigma(const GaussDraw& draw) { return draw.sigma; }
template <int D, int A, class... Rest> __device__ __forceinline__ const Mlp2Net<D, A>& mlp2_net_of(const Mlp2Net<D, A>& net, Rest...) { return net; }
// the lane's four words of step t: one Philox evaluation per lane per step for a head that draws (SAMPLE: a word per environment; GAUSS: a pair per pair of
// environments), zeros for GREEDY, which reads none.  An out-parameter: returned by value, CartPole's greedy kernels came out with another register allocation.
template <int POLICY>
__device__ __forceinline__ void policy_draw(uint64_t seed, uint64_t g, uint32_t call, uint32_t t, Philox4& w) {
    constexpr int HEAD = roll_act_head(POLICY);
    if constexpr (HEAD == MLP_HEAD_GREEDY) w = Philox4{};
    else w = env_draw(seed, g, call, policy_head_slot(HEAD) + t);
}
// from POLICY to net, activation and head, and the one call: `pack` is the kernel's PolicyArg (read by the one-layer sources), `tail` its trailing pack, `sigma`
// the one-layer Gaussian's.  The draw stays at the call site (policy_draw) and its words are handed in: with the draw in here, its arguments by reference or by
// value, the Philox key schedule was hoisted in another order in every kernel that draws.
template <int POLICY, int D, int A, class Pack, class... Tail>
__device__ __forceinline__ void policy_actions4(const Pack& pack, const uint32_t (&w)[4], float sigma, const float (&o)[4][D], uint32_t (&a)[4], const Tail&... tail) {
    constexpr int HEAD = roll_act_head(POLICY), ACT = roll_act_hidden_act(POLICY);
    if constexpr (roll_act_is_mlp2(POLICY)) {
        const Mlp2Net<D, A>& net = mlp2_net_of(tail...);
        mlp_actions<D, A, ACT, HEAD, 4>(net, o, w, net.sigma, a);
    } else {
        mlp_actions<D, A, ACT, HEAD, 4>(pack, o, w, sigma, a);
    }
}

}  // namespace mgym
