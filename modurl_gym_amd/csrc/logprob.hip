// logprob.hip — mgym_logprob_mlp (include/mgym.h): the actor's log-probabilities of a rollout's actions, the words of logprob.h.
//
// One launch, the K x n independent evaluations of logp_out.  Four-per-lane form (n % 4 == 0 and below 2^30, all four device pointers 16-byte aligned), the
// dense kernel of learner.h that mgym_value_mlp's dense pass runs too, here with LogpCall: a lane owns four consecutive environments of one step, loads the row's D components as D 16-byte words and the four action words as
// one more — all issued before the chains — runs mlp_scores<D, A, ACT, 4> with the weights as scalar operands, then the head per environment (the f64 logarithm
// of the softmax sum is one divide and about ten multiply-adds, all selections, no branch on a lane's data), and stores one 16-byte word.  A row's address is a
// wave-uniform 64-bit base plus the lane's 32-bit byte offset; blockIdx.y is the step (steps beyond the grid's 65535 by a stride loop).  Otherwise one environment
// per lane with 64-bit addresses, the same words.  No LDS, no atomics.
#include "learner.h"

namespace mgym {

template <int D, int A, int ACT, class Net>
__global__ void __launch_bounds__(kBlock) logp1_kernel(const Net net, const LogpCall a) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    for (int32_t t = (int32_t)blockIdx.y; t < a.K; t += (int32_t)gridDim.y)
        a.logp_out[(uint64_t)t * a.n + i] = logp_of<D, A, ACT>(net, value_row_in(t, a.n, D, a.obs_first, a.obs), a.n, i, a.actions[(uint64_t)t * a.n + i], a.sigma, a.k);
}

template <int D, int A, int ACT, class Net>
static void launch_form(hipStream_t stream, const LogpCall& c, const Net& net) {
    launch_dense<D, A, ACT>(stream, c, net, four_per_lane(c.n, c.obs_first, c.obs, c.actions, c.logp_out), (unsigned)c.K, logp1_kernel<D, A, ACT, Net>);
}

int logprob_launch(hipStream_t stream, const LogpCall& c, int D, int A, const float* policy, int32_t hidden1, int32_t hidden2, int32_t activation, const float* pack_dev) {
    return with_family(D, A, "mgym_logprob_mlp: no kernels for this family", [&](auto d, auto a) {
        with_net<d.value, a.value>(policy, hidden1, hidden2, pack_dev, c.sigma, [&](const auto& net, auto two) {
            with_activation(activation, two, [&](auto act) { launch_form<d.value, a.value, act.value>(stream, c, net); });
        });
    });
}

}  // namespace mgym
