// grad.hip — mgym_ppo_grad_mlp and mgym_value_grad_mlp (include/mgym.h): a loss and its gradient over a rollout's buffers, the words of grad.h.
//
// Two launches.  The first covers the K x env_count env-steps in tiles of 256 lanes x N environments x S steps (N = 4 with 16-byte rows when n_envs, env_first
// and env_count are multiples of 4, n_envs < 2^30 and every row pointer is 16-byte aligned, else N = 1 with 64-bit addresses; S: kGradFillTiles below).  A lane
// loads its N x S observations, action words and targets, runs mlp_scores once over all of them (weights as scalar operands) and the head per env-step, and
// keeps o and ds in registers.  The second pass walks the hidden units: unit j's pre_j / h_j are recomputed for every env-step of the lane (D fused
// multiply-adds each: cheaper than 64 stored h words per environment), its D + 1 + A terms added by fmaf into the lane's accumulators, which the wave then
// adds across its lanes (four DPP steps inside each row of 16, then the four rows) and lane v adds value v into the wave's own f64 slab in LDS.  At the end
// of its tiles (a block strides over them when there are more tiles than slabs) the block adds its four waves' slabs in wave order and stores one f64 slab to
// the workspace.  The second launch adds the slabs in index order in f64, scales by 1 / B, rounds to f32 and writes grad_out and stats_out.  No atomics, no
// tickets: the order of every sum is a function of the arguments alone.  A word outside the environments' range or beyond step K - 1 is never loaded.
#include "learner.h"

namespace mgym {

constexpr int kGradWaves = kBlock / 64;
static_assert(kGradWaves == 4, "the block's last sum names its four waves' slabs");

// Steps of its environments a lane takes before each wave reduction: the registers hold N x S x (D + A) words of o and ds, and the heads of all N x S
// env-steps are in flight together.  Four environments per lane: 2 steps when that gives at least kGradFillTiles tiles, else 1 — measured (DESIGN.md 5i:
// three builds in one session): at 1 Mi environments, K = 16 (8 192 tiles) 1 step is 4 - 28 % slower than 2, the wave sums shared by twice the terms; at
// 4 096 environments (32 tiles on 256 compute units) 1 step is up to 36 % faster (one row of 24 equal), twice the blocks at half the serial work each.  Between those two sizes the
// threshold is a choice, the chip's compute units, not a measurement.  4 steps were not timed: the (4, 2) kernels then take 219 - 251 VGPRs and the (2, 3),
// (6, 3) and (8, 4) ones a private segment (profiles/grad_kernel_resources.txt).  One environment per lane: 4 steps, not measured against others.
// (make EXTRA=-DGRAD_STEPS4=1 or 2 builds one count for every size: the builds of that measurement.)
constexpr uint64_t kGradFillTiles = 256;
constexpr int kGradSteps1 = 4;

// (the wave sum, grad_wave_sum, is learner.h's: the two-layer kernels of grad2.hip take their tails through it too)

template <int D, int A, int ACT, class Head, int N, int S>
__global__ void __launch_bounds__(kBlock) grad_kernel(const MlpPack<D, A> net, const Head head, const GradCall c) {
    constexpr int V = D + 1 + A, E = N * S, T = A + 1 + kGradStats, WMAX = D * kMlpMaxHidden + kMlpMaxHidden + A * (kMlpMaxHidden + 1) + kGradTail;
    static_assert(V <= 64 && T <= 64, "one lane per reduced value");
    __shared__ double slab[kGradWaves][WMAX];
    const int H = net.hidden, P = mlp_policy_floats(D, A, H), W = P + kGradTail;
    for (int i = (int)threadIdx.x; i < kGradWaves * WMAX; i += kBlock) (&slab[0][0])[i] = 0.0;
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    // where lane v's value of unit j stands: dW1[j][v], db1[j], dW2[v - D - 1][j]
    const int unit_base = lane < D ? lane : (lane == D ? H * D : H * D + H + (lane - D - 1) * H), unit_stride = lane < D ? D : 1;
    double* mine_slab = slab[wave];
    const uint64_t lanes = (c.env_count + N - 1) / N, tiles_x = (lanes + kBlock - 1) / kBlock;
    const uint64_t tiles = tiles_x * (uint64_t)((c.K + S - 1) / S);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // block-uniform
        const int32_t t0 = (int32_t)(tile / tiles_x) * S;
        const int steps = c.K - t0 < S ? c.K - t0 : S;
        const uint64_t q = (tile % tiles_x) * kBlock + threadIdx.x;
        const bool in = q < lanes;
        const uint64_t i0 = c.env_first + q * N;   // (in: i0 + N <= env_first + env_count <= n)
        float o[E][D], ds[E][A], tail[T];
#pragma unroll
        for (int v = 0; v < T; ++v) tail[v] = 0.0f;
        {
            uint32_t w[E];
            float x0[E], x1[E];
#pragma unroll
            for (int st = 0; st < S; ++st) {
                const bool live = in && st < steps;
                float ob[D][N], a0[N], a1[N];
                uint32_t aw[N];
#pragma unroll
                for (int k = 0; k < N; ++k) { a0[k] = 0.0f; a1[k] = 0.0f; aw[k] = 0u; }
#pragma unroll
                for (int d = 0; d < D; ++d)
#pragma unroll
                    for (int k = 0; k < N; ++k) ob[d][k] = 0.0f;
                if (live) {
                    const int32_t t = t0 + st;
                    const float* row = value_row_in(t, c.n, D, c.obs_first, c.obs);
#pragma unroll
                    for (int d = 0; d < D; ++d) grad_load<N>(row + (uint64_t)d * c.n, i0, ob[d]);
                    grad_load<N>(c.x0 + (uint64_t)t * c.n, i0, a0);
                    if constexpr (Head::kPpo) {
                        grad_load<N>(c.actions + (uint64_t)t * c.n, i0, aw);
                        grad_load<N>(c.x1 + (uint64_t)t * c.n, i0, a1);
                    }
                }
#pragma unroll
                for (int k = 0; k < N; ++k) {
#pragma unroll
                    for (int d = 0; d < D; ++d) o[st * N + k][d] = ob[d][k];
                    w[st * N + k] = aw[k]; x0[st * N + k] = a0[k]; x1[st * N + k] = a1[k];
                }
            }
            float s[E][A];
            mlp_scores<D, A, ACT, E>(net, o, s);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const bool live = in && e / N < steps;
                GradStep<A> g;
                head.step(s[e], w[e], x0[e], x1[e], g);
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    ds[e][a] = live ? g.ds[a] : 0.0f;
                    tail[a] += ds[e][a];
                }
                tail[A] += live ? g.dls : 0.0f;
#pragma unroll
                for (int k = 0; k < kGradStats; ++k) tail[A + 1 + k] += live ? g.stat[k] : 0.0f;
            }
        }
        for (int j = 0; j < H; ++j) {
            const float* u = net.unit[j];
            float acc[V];
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = 0.0f;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (e / N < steps) {   // block-uniform
                    float h, dpre;
                    grad_unit<D, A, ACT>(u, o[e], ds[e], &h, &dpre);
#pragma unroll
                    for (int d = 0; d < D; ++d) acc[d] = cp_fmaf(dpre, o[e][d], acc[d]);
                    acc[D] += dpre;
#pragma unroll
                    for (int a = 0; a < A; ++a) acc[D + 1 + a] = cp_fmaf(ds[e][a], h, acc[D + 1 + a]);
                }
            }
            float mine = 0.0f;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float r = grad_wave_sum(acc[v]);
                mine = lane == v ? r : mine;
            }
            if (lane < V) mine_slab[unit_base + j * unit_stride] += (double)mine;
        }
        float mine = 0.0f;
#pragma unroll
        for (int v = 0; v < T; ++v) {
            const float r = grad_wave_sum(tail[v]);
            mine = lane == v ? r : mine;
        }
        if (lane < T) mine_slab[P - A + lane] += (double)mine;   // db2[0 .. A-1], the log-sigma sum, the five statistics' sums
    }
    __syncthreads();
    double* out = c.workspace + (uint64_t)blockIdx.x * (uint64_t)W;
    for (int i = (int)threadIdx.x; i < W; i += kBlock) out[i] = ((slab[0][i] + slab[1][i]) + slab[2][i]) + slab[3][i];
}

// the slabs added in index order, scaled and rounded: grad_out[0 .. P], stats_out[0 .. 7]
__global__ void __launch_bounds__(kBlock) grad_finish_kernel(const double* ws, int slabs, int P, double B, float ent_coef, int gauss, float* grad_out, float* stats_out) {
    const int out = (int)(blockIdx.x * kBlock + threadIdx.x), W = P + kGradTail;
    if (out > P + kGradTail) return;
    double sum = 0.0;
    if (out <= P + kGradStats)
        for (int s = 0; s < slabs; ++s) sum += ws[(uint64_t)s * (uint64_t)W + (uint64_t)out];
    const float r = grad_result(sum, P, out, B, ent_coef, gauss != 0);
    if (out <= P) grad_out[out] = r;
    else stats_out[out - (P + 1)] = r;
}

void grad_finish_launch(hipStream_t stream, const GradCall& c, int slabs, int P, bool gauss) {
    hipLaunchKernelGGL(grad_finish_kernel, dim3((unsigned)((P + kGradTail + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, c.workspace, slabs, P,
                       (double)c.K * (double)c.env_count, c.ent_coef, gauss ? 1 : 0, c.grad_out, c.stats_out);
}

template <int D, int A, int ACT, class Head>
static void launch_form(hipStream_t stream, const GradCall& c, const MlpPack<D, A>& net, const Head& head) {
    const bool four = grad_four_per_lane(c, Head::kPpo);
    const int N = four ? 4 : 1;
#if defined(GRAD_STEPS4)
    const bool two = GRAD_STEPS4 == 2;
#else
    const bool two = grad_tiles(c, N, 2) >= kGradFillTiles;
#endif
    const unsigned blocks = grad_blocks(c, N, four ? (two ? 2 : 1) : kGradSteps1);
    if (four && two) hipLaunchKernelGGL((grad_kernel<D, A, ACT, Head, 4, 2>), dim3(blocks), dim3(kBlock), 0, stream, net, head, c);
    else if (four) hipLaunchKernelGGL((grad_kernel<D, A, ACT, Head, 4, 1>), dim3(blocks), dim3(kBlock), 0, stream, net, head, c);
    else hipLaunchKernelGGL((grad_kernel<D, A, ACT, Head, 1, kGradSteps1>), dim3(blocks), dim3(kBlock), 0, stream, net, head, c);
    grad_finish_launch(stream, c, (int)blocks, mlp_policy_floats(D, A, net.hidden), std::is_same<Head, PpoGaussian>::value);
}

template <int D, int A, class Head>
static void launch_act(hipStream_t stream, const GradCall& c, const Head& head, const float* weights, int32_t hidden, int32_t act) {
    MlpPack<D, A> pack;
    mlp_pack<D, A>(weights, hidden, pack);
    with_activation(act, std::false_type{}, [&](auto ACT) { launch_form<D, A, ACT.value>(stream, c, pack, head); });
}

int grad_launch(hipStream_t stream, const GradCall& c, int D, int A, int head, const float* weights, int32_t hidden, int32_t activation) {
    return with_family(D, A, "mgym gradient call: no kernels for this family", [&](auto d, auto a) {
        const PpoTerms terms{c.lo, c.hi, c.ent_coef};
        if (head == GRAD_HEAD_VALUE) launch_act<d.value, 1>(stream, c, ValueMse{}, weights, hidden, activation);
        else if constexpr (a.value == 1) launch_act<d.value, 1>(stream, c, PpoGaussian{terms, c.sigma, c.k, c.ent}, weights, hidden, activation);
        else launch_act<d.value, a.value>(stream, c, PpoCategorical<a.value>{terms}, weights, hidden, activation);
    });
}

}  // namespace mgym
