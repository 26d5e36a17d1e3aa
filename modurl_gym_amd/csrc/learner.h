// learner.h — what the learner calls over a rollout's buffers share: mgym_value_mlp (value.hip), mgym_logprob_mlp (logprob.hip) and the two gradient calls
// (grad.hip).  The way from run-time (D, A), activation and depth to template arguments, the four-per-lane predicate and caps, and the one four-per-lane dense
// kernel of the value and log-probability calls.  Included by those three files (and free to abi.hip) only: no other translation unit's kernels see it.
#pragma once
#include "common.h"
#include "grad.h"

namespace mgym {

constexpr uint64_t kFourMaxEnvs = 1ull << 30;   // the four-per-lane kernel addresses a row by a 32-bit byte offset
constexpr unsigned kMaxGridY = 65535u;
inline unsigned grid_rows(unsigned rows) { return rows < kMaxGridY ? rows : kMaxGridY; }   // blockIdx.y is the row; rows beyond the grid's by a stride loop

// may a lane own four consecutive environments of a row: n % 4 == 0, n below the cap, and every listed row pointer 16-byte aligned (a null one is)
template <class... P>
inline bool four_per_lane(uint64_t n, const P*... rows) { return n % 4 == 0 && n < kFourMaxEnvs && (aligned(rows, 16) && ...); }

// The launch shape of a gradient call of either depth (grad.hip, grad2.hip).  Four environments per lane: every row the kernel loads 16 bytes at a time aligned
// and the range a whole number of fours; the tiles of 256 lanes x N environments x S steps over K x env_count env-steps; one block per tile up to the slabs
inline bool grad_four_per_lane(const GradCall& c, bool ppo) {
    return four_per_lane(c.n, c.obs_first, c.obs, c.x0) && c.env_first % 4 == 0 && c.env_count % 4 == 0 && (!ppo || (aligned(c.actions, 16) && aligned(c.x1, 16)));
}
inline uint64_t grad_tiles(const GradCall& c, int N, int S) {
    const uint64_t lanes = (c.env_count + N - 1) / N;
    return ((lanes + kBlock - 1) / kBlock) * (uint64_t)((c.K + S - 1) / S);
}
inline unsigned grad_blocks(const GradCall& c, int N, int S) {
    const uint64_t tiles = grad_tiles(c, N, S);
    return (unsigned)(tiles < (uint64_t)c.slabs ? tiles : (uint64_t)c.slabs);
}

// The by-value kernel arguments of every learner kernel, against the largest net and the largest call struct (the actor's gradient call with its head).
static_assert(sizeof(MlpPack<8, 1>) == 2568 && sizeof(MlpPack<8, 4>) == 3348 && sizeof(ValueCall) <= sizeof(GradCall) && sizeof(LogpCall) <= sizeof(GradCall) &&
                  sizeof(MlpPack<8, 4>) + sizeof(PpoGaussian) + sizeof(GradCall) + 16 <= 4096,
              "learner kernels: by-value kernel arguments above 4096 bytes");

template <int N>
using Int = std::integral_constant<int, N>;

// The one way from a family's run-time (D, A) to template arguments: f(Int<D>{}, Int<A>{}) for the six families.  A == 0 asks by D alone (the critic's call: one
// score whatever the family's actions; f then ignores A, and (2, 1) and (2, 3) share D).  `none`: the caller's error text for an unknown pair.  f launches:
// the status is its launches'.
template <class F>
int with_family(int D, int A, const char* none, F&& f) {
    switch (D * 10 + A) {
    case 40: case 42: f(Int<4>{}, Int<2>{}); break;   // CartPole
    case 20: case 23: f(Int<2>{}, Int<3>{}); break;   // MountainCar
    case 21: f(Int<2>{}, Int<1>{}); break;            // MountainCarContinuous
    case 30: case 31: f(Int<3>{}, Int<1>{}); break;   // Pendulum
    case 60: case 63: f(Int<6>{}, Int<3>{}); break;   // Acrobot
    case 80: case 84: f(Int<8>{}, Int<4>{}); break;   // LunarLander
    default: set_last_error(none); return MGYM_ERR_BAD_ARG;
    }
    MGYM_HIP(hipGetLastError());
    return MGYM_OK;
}

// f(Int<ACT>{}) for a checked activation; two_layers (a std::bool_constant: the exact tanh is not instantiated there) offers no exact tanh
template <class Two, class F>
void with_activation(int32_t act, Two two_layers, F&& f) {
    if (act == MLP_ACT_RELU) return f(Int<MLP_ACT_RELU>{});
    if constexpr (!Two::value)
        if (act == MLP_ACT_TANH) return f(Int<MLP_ACT_TANH>{});
    f(Int<MLP_ACT_TANH_FAST>{});
}

// f(net, two_layers) with the net the kernels take: h2 == 0: the caller's host words by value as an MlpPack<D, A>, else an Mlp2Net<D, A> on `pack_dev`, the
// handle's device pack, which holds them by then (Env::mlp2_store_to)
template <int D, int A, class F>
void with_net(const float* weights, int32_t h1, int32_t h2, const float* pack_dev, float sigma, F&& f) {
    if (h2 == 0) {
        MlpPack<D, A> pack;
        mlp_pack<D, A>(weights, h1, pack);
        f(pack, std::false_type{});
    } else {
        f(Mlp2Net<D, A>{pack_dev, h1, h2, sigma}, std::true_type{});
    }
}

#if defined(__HIPCC__)
template <class V, class T>
__device__ __forceinline__ V& word_at(T* row, uint32_t off) {
    typedef typename std::conditional<std::is_const<T>::value, const char, char>::type Byte;
    return *reinterpret_cast<V*>(reinterpret_cast<Byte*>(row) + off);
}

// ---- the gradient kernels' wave sum (grad.hip, grad2.hip) ----
#if defined(GRAD_WAVE_SHFL)
// (make EXTRA=-DGRAD_WAVE_SHFL: the same sum through six ds_bpermute butterflies.  Measured against the DPP form below in one session, DESIGN.md 5i: between
// equal within 1 % and 26 % slower on the actor's rows, 1 - 4 % faster on the critic's tanh_fast rows only; not kept)
__device__ __forceinline__ float grad_wave_sum(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
#else
template <int CTRL>
__device__ __forceinline__ float grad_dpp(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
// the sum of x over the wave's 64 lanes, the same word in every lane; all 64 lanes are active at every call.  quad_perm [1,0,3,2] and [2,3,0,1] leave every
// lane of a quad with the quad's sum, row_half_mirror every lane of 8 with the sum of its two quads, row_mirror every lane of a row of 16 with the row's
// sum (each step adds two values that both sides hold, so both get the same word); the four rows' sums are then read as scalars and added in row order
__device__ __forceinline__ float grad_wave_sum(float x) {
    x += grad_dpp<0xB1>(x);
    x += grad_dpp<0x4E>(x);
    x += grad_dpp<0x141>(x);
    x += grad_dpp<0x140>(x);
    const int xi = __float_as_int(x);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(xi, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(xi, 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(xi, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(xi, 48));
    return ((r0 + r1) + r2) + r3;
}
#endif

// N words of row `row` ([n] each) at environments i .. i + N - 1 (the gradient kernels); the four-per-lane form by one 16-byte load at a 32-bit byte offset
template <int N, class T>
__device__ __forceinline__ void grad_load(const T* row, uint64_t i, T (&out)[N]) {
    if constexpr (N == 4) {
        typedef typename std::conditional<std::is_same<T, float>::value, float4, uint4>::type V4;
        const V4 v = word_at<const V4>(row, (uint32_t)i * 4u);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else {
        out[0] = row[i];
    }
}

// The four-per-lane dense pass of mgym_value_mlp and mgym_logprob_mlp (n % 4 == 0 and below 2^30, the rows 16-byte aligned): a lane owns four consecutive
// environments of one row, loads the row's D components as D 16-byte words — and, where the call has actions, the four action words as one more, all issued
// before the chains — runs mlp_scores<D, A, ACT, 4> with the weights as scalar operands, and stores one 16-byte word.  A row's address is a wave-uniform 64-bit
// base plus the lane's 32-bit byte offset; blockIdx.y is the row (grid_rows).  The call struct says how many rows (rows()), where row r goes (out_row(r)),
// whether it has an action row (kActions, action_row(r)) and the word an environment's scores and action word make (word<A>(s, w)).
// (The one-per-lane kernels stay in their files: no shared form of them reproduced the separate ones to the instruction.)
template <int D, int A, int ACT, class Net, class Call>
__global__ void __launch_bounds__(kBlock) dense4_kernel(const Net net, const Call a) {
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;   // (n < 2^30: lanes and byte offsets fit 32 bits)
    if (lane >= (uint32_t)(a.n / 4)) return;
    const uint32_t off16 = lane * 16u;
    for (int32_t r = (int32_t)blockIdx.y; r < a.rows(); r += (int32_t)gridDim.y) {   // wave-uniform
        const float* in = value_row_in(r, a.n, D, a.obs_first, a.obs);
        float4 c[D];
#pragma unroll
        for (int q = 0; q < D; ++q) c[q] = word_at<const float4>(in + (uint64_t)q * a.n, off16);
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (Call::kActions) w = word_at<const uint4>(a.action_row(r), off16);
        float o[4][D], s[4][A];
#pragma unroll
        for (int q = 0; q < D; ++q) { o[0][q] = c[q].x; o[1][q] = c[q].y; o[2][q] = c[q].z; o[3][q] = c[q].w; }
        mlp_scores<D, A, ACT, 4>(net, o, s);
        word_at<float4>(a.out_row(r), off16) = make_float4(a.template word<A>(s[0], w.x), a.template word<A>(s[1], w.y), a.template word<A>(s[2], w.z), a.template word<A>(s[3], w.w));
    }
}

// the dense launch of a call: the four-per-lane kernel above where `four`, else the file's own one-per-lane kernel `one`, on the same rows
template <int D, int A, int ACT, class Net, class Call, class One>
void launch_dense(hipStream_t stream, const Call& c, const Net& net, bool four, unsigned rows, One one) {
    if (four) hipLaunchKernelGGL((dense4_kernel<D, A, ACT, Net, Call>), dim3((unsigned)((c.n / 4 + kBlock - 1) / kBlock), grid_rows(rows)), dim3(kBlock), 0, stream, net, c);
    else hipLaunchKernelGGL(one, dim3((unsigned)((c.n + kBlock - 1) / kBlock), grid_rows(rows)), dim3(kBlock), 0, stream, net, c);
}
#endif

}  // namespace mgym
