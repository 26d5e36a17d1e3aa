// logprob.hip — mgym_logprob_mlp (include/mgym.h): the actor's log-probabilities of a rollout's actions, the words of logprob.h.
//
// One launch, the K x n independent evaluations of logp_out, shaped as value.hip's dense pass.  Four-per-lane form (n % 4 == 0 and below 2^30, all four device
// pointers 16-byte aligned): a lane owns four consecutive environments of one step, loads the row's D components as D 16-byte words and the four action words as
// one more — all issued before the chains — runs mlp_scores<D, A, ACT, 4> with the weights as scalar operands, then the head per environment (the f64 logarithm
// of the softmax sum is one divide and about ten multiply-adds, all selections, no branch on a lane's data), and stores one 16-byte word.  A row's address is a
// wave-uniform 64-bit base plus the lane's 32-bit byte offset; blockIdx.y is the step (steps beyond the grid's 65535 by a stride loop).  Otherwise one environment
// per lane with 64-bit addresses, the same words.  No LDS, no atomics.
#include "common.h"
#include "logprob.h"

namespace mgym {

template <class V, class T>
__device__ __forceinline__ V& logp_word_at(T* row, uint32_t off) {
    typedef typename std::conditional<std::is_const<T>::value, const char, char>::type Byte;
    return *reinterpret_cast<V*>(reinterpret_cast<Byte*>(row) + off);
}

template <int D, int A, int ACT, class Net>
__global__ void __launch_bounds__(kBlock) logp4_kernel(const Net net, const LogpCall a) {
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;   // (n < 2^30: lanes and byte offsets fit 32 bits)
    if (lane >= (uint32_t)(a.n / 4)) return;
    const uint32_t off16 = lane * 16u;
    for (int32_t t = (int32_t)blockIdx.y; t < a.K; t += (int32_t)gridDim.y) {   // wave-uniform
        const float* in = value_row_in(t, a.n, D, a.obs_first, a.obs);
        float4 c[D];
#pragma unroll
        for (int q = 0; q < D; ++q) c[q] = logp_word_at<const float4>(in + (uint64_t)q * a.n, off16);
        const uint4 w = logp_word_at<const uint4>(a.actions + (uint64_t)t * a.n, off16);
        float o[4][D], s[4][A];
#pragma unroll
        for (int q = 0; q < D; ++q) { o[0][q] = c[q].x; o[1][q] = c[q].y; o[2][q] = c[q].z; o[3][q] = c[q].w; }
        mlp_scores<D, A, ACT, 4>(net, o, s);
        logp_word_at<float4>(a.logp_out + (uint64_t)t * a.n, off16) = make_float4(logp_head<A>(s[0], w.x, a.sigma, a.k), logp_head<A>(s[1], w.y, a.sigma, a.k),
                                                                                  logp_head<A>(s[2], w.z, a.sigma, a.k), logp_head<A>(s[3], w.w, a.sigma, a.k));
    }
}

template <int D, int A, int ACT, class Net>
__global__ void __launch_bounds__(kBlock) logp1_kernel(const Net net, const LogpCall a) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    for (int32_t t = (int32_t)blockIdx.y; t < a.K; t += (int32_t)gridDim.y)
        a.logp_out[(uint64_t)t * a.n + i] = logp_of<D, A, ACT>(net, value_row_in(t, a.n, D, a.obs_first, a.obs), a.n, i, a.actions[(uint64_t)t * a.n + i], a.sigma, a.k);
}

constexpr uint64_t kLogpFourMaxEnvs = 1ull << 30;   // the four-per-lane kernel addresses a row by a 32-bit byte offset
constexpr unsigned kLogpMaxGridY = 65535u;

template <int D, int A, int ACT, class Net>
static void launch_form(hipStream_t stream, const LogpCall& c, const Net& net) {
    const bool four = c.n % 4 == 0 && c.n < kLogpFourMaxEnvs && aligned(c.obs_first, 16) && aligned(c.obs, 16) && aligned(c.actions, 16) && aligned(c.logp_out, 16);
    const unsigned rows = (unsigned)c.K < kLogpMaxGridY ? (unsigned)c.K : kLogpMaxGridY;
    if (four) hipLaunchKernelGGL((logp4_kernel<D, A, ACT, Net>), dim3((unsigned)((c.n / 4 + kBlock - 1) / kBlock), rows), dim3(kBlock), 0, stream, net, c);
    else hipLaunchKernelGGL((logp1_kernel<D, A, ACT, Net>), dim3((unsigned)((c.n + kBlock - 1) / kBlock), rows), dim3(kBlock), 0, stream, net, c);
}

template <int D, int A>
static void launch_family(hipStream_t stream, const LogpCall& c, const float* policy, int32_t h1, int32_t h2, int32_t act, const float* pack_dev) {
    if (h2 == 0) {
        static_assert(sizeof(MlpPack<8, 4>) == 3348 && sizeof(MlpPack<8, 4>) + sizeof(LogpCall) + 16 <= 4096, "logprob kernels: by-value kernel arguments above 4096 bytes");
        MlpPack<D, A> pack;
        mlp_pack<D, A>(policy, h1, pack);
        if (act == MLP_ACT_RELU) launch_form<D, A, MLP_ACT_RELU>(stream, c, pack);
        else if (act == MLP_ACT_TANH) launch_form<D, A, MLP_ACT_TANH>(stream, c, pack);
        else launch_form<D, A, MLP_ACT_TANH_FAST>(stream, c, pack);
    } else {
        const Mlp2Net<D, A> net{pack_dev, h1, h2, c.sigma};
        if (act == MLP_ACT_RELU) launch_form<D, A, MLP_ACT_RELU>(stream, c, net);
        else launch_form<D, A, MLP_ACT_TANH_FAST>(stream, c, net);
    }
}

int logprob_launch(hipStream_t stream, const LogpCall& c, int D, int A, const float* policy, int32_t hidden1, int32_t hidden2, int32_t activation, const float* pack_dev) {
    const int key = D * 10 + A;
    switch (key) {
    case 42: launch_family<4, 2>(stream, c, policy, hidden1, hidden2, activation, pack_dev); break;   // CartPole
    case 23: launch_family<2, 3>(stream, c, policy, hidden1, hidden2, activation, pack_dev); break;   // MountainCar
    case 21: launch_family<2, 1>(stream, c, policy, hidden1, hidden2, activation, pack_dev); break;   // MountainCarContinuous
    case 31: launch_family<3, 1>(stream, c, policy, hidden1, hidden2, activation, pack_dev); break;   // Pendulum
    case 63: launch_family<6, 3>(stream, c, policy, hidden1, hidden2, activation, pack_dev); break;   // Acrobot
    case 84: launch_family<8, 4>(stream, c, policy, hidden1, hidden2, activation, pack_dev); break;   // LunarLander
    default: set_last_error("mgym_logprob_mlp: no kernels for this family"); return MGYM_ERR_BAD_ARG;
    }
    MGYM_HIP(hipGetLastError());
    return MGYM_OK;
}

}  // namespace mgym
