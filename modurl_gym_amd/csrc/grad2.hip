// grad2.hip — mgym_ppo_grad_mlp2 and mgym_value_grad_mlp2 (include/mgym.h): grad.hip's calls for the two-hidden-layer net, the words of grad2.h.
//
// Two launches, as in grad.hip.  The first covers the K x env_count env-steps in tiles of 256 lanes x 4 env-steps: four environments of one step where
// n_envs, env_first and env_count are multiples of 4, n_envs < 2^30 and every row pointer is 16-byte aligned (16-byte loads), else one environment at four
// steps (64-bit addresses).  A lane takes its four env-steps one after the other.  For one env-step it runs layer 1 (h1 stays in registers), the units of
// layer 2 for the scores, and the head (pass 1); then the units of layer 2 again (pass 2): pre2_k / h2_k recomputed from h1 (H1 multiply-adds: cheaper than
// 64 more registers beside h1 and dh1), dpre2_k formed, and the dh1 chain advanced across all j.  Everything word-defined is a VALU chain of the lane with the
// weights as scalar operands of the handle's pack, the forward's own chains.
//
// The sums over the batch are matrix products whose contraction index is the lane, so they go to the f32 matrix pipe (v_mfma_f32_16x16x4_f32, exact f32
// products): a wave stages its 64 env-steps' words in LDS as [word][env-step] rows (stride 68 words: a lane's store and the operand reads, 16 rows x 4
// env-steps, both touch 64 different banks) — h1 (64 rows), the tile E = [o_0 .. o_{D-1}, 1, ds_0 .. ds_{A-1}, 0 ..] (16 rows), and 16 units of dpre2 and
// of h2 at a time as pass 2 produces them.  Per chunk of 16 units and per group of 4 env-steps, dpre2 x h1 gives dW2, dpre2 x E gives db2 (the column of
// ones), h2 x E gives dW3 (the columns of ds); after pass 2, dpre1 x E gives dW1 and db1.  The accumulators (112 registers) carry f32 over two env-steps
// per lane, 128 of the wave; then the four waves add them, in wave order, into the block's one f64 slab in LDS (per-wave slabs as in grad.hip do not fit
// beside the staging).  The tail — db3, the log-sigma sum, the statistics' sums — goes through learner.h's wave sum per env-step and then in f64 per wave.
// A block strides over the tiles when there are more tiles than slabs and stores its slab to the workspace at the end; the second launch is grad.hip's
// grad_finish_kernel.  No atomics, no tickets: the order of every sum is a function of the arguments alone.  A word outside the environments' range or
// beyond step K - 1 is never loaded; a lane without an env-step stages zeros.
#include "learner.h"
#include "grad2.h"

namespace mgym {

constexpr int kG2Waves = kBlock / 64;
constexpr int kG2Stride = 68;                                  // words of a staged row: 64 env-steps and 4 of padding
constexpr int kG2RowsH1 = kMlpMaxHidden, kG2Tile = 16;         // rows of h1, and of every other staged tile
constexpr int kG2StageWords = (kG2RowsH1 + 3 * kG2Tile) * kG2Stride;   // h1, E, the chunk of dpre2 (then dpre1), the chunk of h2
constexpr int kG2Steps = 4;                                    // env-steps of a lane in a tile
constexpr int kG2Carry = 2;                                    // of which the f32 accumulators carry this many before the f64 slab
static_assert(kG2Waves == 4 && kMlpMaxHidden == 64, "four waves, four chunks of 16 units");

typedef float g2_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ g2_f4 g2_mfma(float a, float b, g2_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// the wave's staged words are read by other lanes than wrote them: orders the LDS accesses around it, in the compiler and in the wave
__device__ __forceinline__ void g2_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
MG_HD Mlp2Ptr g2_pack(const float* pack) { return mlp2_const(pack); }   // (mlp2_const is a host function in the host pass: reached through a two-sided one)
__device__ __forceinline__ float g2_pick(const float (&v)[kG2Steps], int e) { return e == 0 ? v[0] : (e == 1 ? v[1] : (e == 2 ? v[2] : v[3])); }
__device__ __forceinline__ uint32_t g2_pick(const uint32_t (&v)[kG2Steps], int e) { return e == 0 ? v[0] : (e == 1 ? v[1] : (e == 2 ? v[2] : v[3])); }

template <int D, int A, int ACT, class Head, int N>
__global__ void __launch_bounds__(kBlock) grad2_kernel(const Mlp2Net<D, A> net, const Head head, const GradCall c) {
    constexpr int S = kG2Steps / N, E = kG2Steps, T = A + 1 + kGradStats, WMAX = mlp2_policy_floats(D, A, kMlpMaxHidden, kMlpMaxHidden) + kGradTail;
    static_assert(N == 1 || N == 4, "one environment at four steps, or four environments at one");
    static_assert(D + 1 + A <= kG2Tile && T <= kG2Tile, "the tile E is one tile; a lane per word of the tail");
    __shared__ double slab[WMAX];
    __shared__ float stage[kG2Waves][kG2StageWords];
    __shared__ double tails[kG2Waves][kG2Tile];   // each wave's f64 sums of the tail's T words
    const int H1 = net.h1, H2 = net.h2, P = mlp2_policy_floats(D, A, H1, H2), W = P + kGradTail;
    for (int i = (int)threadIdx.x; i < W; i += kBlock) slab[i] = 0.0;
    for (int i = (int)threadIdx.x; i < kG2Waves * kG2StageWords; i += kBlock) (&stage[0][0])[i] = 0.0f;   // (rows of units beyond the widths are read, their products dropped)
    if (threadIdx.x < kG2Waves * kG2Tile) (&tails[0][0])[threadIdx.x] = 0.0;
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    float* const h1T = stage[wave];
    float* const eT = h1T + kG2RowsH1 * kG2Stride;
    float* const c1 = eT + kG2Tile * kG2Stride;
    float* const c2 = c1 + kG2Tile * kG2Stride;
    const int r16 = lane & 15, kq = lane >> 4;
    const int rd = r16 * kG2Stride + kq;   // a lane's operand word of a tile, group of env-steps b0: [row r16][4 b0 + kq]
    const Mlp2Ptr p = g2_pack(net.pack);
    const int l2 = mlp2_l2_offset(D, H1), stride = mlp2_l2_stride(H1);
    const int full = H1 & ~7, rem = H1 & 7;   // the whole chunks of 8 units of layer 1, and the units of its last, partial chunk (mlp2_policy.h)
    const int tiles1 = (H1 + 15) >> 4, tiles2 = (H2 + 15) >> 4;
    const uint64_t lanes = (c.env_count + N - 1) / N, tiles_x = (lanes + kBlock - 1) / kBlock;
    const uint64_t tiles = tiles_x * (uint64_t)((c.K + S - 1) / S);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // block-uniform
        const int32_t t0 = (int32_t)(tile / tiles_x) * S;
        const int steps = c.K - t0 < S ? c.K - t0 : S;
        const uint64_t q = (tile % tiles_x) * kBlock + threadIdx.x;
        const bool in = q < lanes;
        const uint64_t i0 = c.env_first + q * N;   // (in: i0 + N <= env_first + env_count <= n)
        float o4[D][E], x04[E], x14[E];
        uint32_t w4[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            x04[e] = 0.0f; x14[e] = 0.0f; w4[e] = 0u;
#pragma unroll
            for (int d = 0; d < D; ++d) o4[d][e] = 0.0f;
        }
#pragma unroll
        for (int st = 0; st < S; ++st) {
            if (in && st < steps) {
                const int32_t t = t0 + st;
                const float* row = value_row_in(t, c.n, D, c.obs_first, c.obs);
                float v[N];
                uint32_t vw[N];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    grad_load<N>(row + (uint64_t)d * c.n, i0, v);
#pragma unroll
                    for (int k = 0; k < N; ++k) o4[d][st * N + k] = v[k];
                }
                grad_load<N>(c.x0 + (uint64_t)t * c.n, i0, v);
#pragma unroll
                for (int k = 0; k < N; ++k) x04[st * N + k] = v[k];
                if constexpr (Head::kPpo) {
                    grad_load<N>(c.actions + (uint64_t)t * c.n, i0, vw);
                    grad_load<N>(c.x1 + (uint64_t)t * c.n, i0, v);
#pragma unroll
                    for (int k = 0; k < N; ++k) { w4[st * N + k] = vw[k]; x14[st * N + k] = v[k]; }
                }
            }
        }
#pragma unroll 1
        for (int e0 = 0; e0 < E; e0 += kG2Carry) {
            g2_f4 acc2[4][4], accb2[4], acc3[4], acc1[4];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                accb2[cc] = acc3[cc] = acc1[cc] = g2_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc2[cc][nt] = g2_f4{0.0f, 0.0f, 0.0f, 0.0f};
            }
#pragma unroll 1
            for (int e = e0; e < e0 + kG2Carry; ++e) {
                const bool live = in && e / N < steps;
                float o[D];
#pragma unroll
                for (int d = 0; d < D; ++d) o[d] = g2_pick(o4[d], e);
                // ---- pass 1: layer 1 (staged as it is made), the scores, the head ----
                float h1[kMlpMaxHidden], ht[7];   // units 0 .. full - 1, and units full .. H1 - 1: indexed statically everywhere (mlp2_policy.h)
#pragma unroll
                for (int cb = 0; cb < kMlpMaxHidden; cb += 8) {
                    if (cb >= full) break;   // wave-uniform
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) {
                        if (cb + jj >= H1) break;
                        h1[cb + jj] = mlp2_hidden1<D, ACT>(p + kMlp2Head + (cb + jj) * (D + 1), o);
                        h1T[(cb + jj) * kG2Stride + lane] = h1[cb + jj];
                        MLP2_ORDER();
                    }
                }
#pragma unroll
                for (int jj = 0; jj < 7; ++jj) {
                    if (jj >= rem) break;
                    ht[jj] = mlp2_hidden1<D, ACT>(p + kMlp2Head + (full + jj) * (D + 1), o);
                    h1T[(full + jj) * kG2Stride + lane] = ht[jj];
                    MLP2_ORDER();
                }
                // unit k's pre-activation: the forward's chain, whole chunks of 8 and the unpadded tail
                const auto pre2_of = [&](const Mlp2Ptr u) __attribute__((always_inline)) {
                    float pre = u[0];
#pragma unroll
                    for (int cb = 0; cb < kMlpMaxHidden; cb += 8) {
                        if (cb >= full) break;
#pragma unroll
                        for (int jj = 0; jj < 8; ++jj) pre = cp_fmaf(u[kMlp2Head + cb + jj], h1[cb + jj], pre);
                        MLP2_ORDER();
                    }
#pragma unroll
                    for (int jj = 0; jj < 7; ++jj) {
                        if (jj >= rem) break;
                        pre = cp_fmaf(u[kMlp2Head + full + jj], ht[jj], pre);
                    }
                    return pre;
                };
                float s[A];
#pragma unroll
                for (int a = 0; a < A; ++a) s[a] = p[a];
                for (int k = 0; k < H2; ++k) {
                    const Mlp2Ptr u = p + l2 + k * stride;
                    const float h2 = mlp_activate<ACT>(pre2_of(u));
#pragma unroll
                    for (int a = 0; a < A; ++a) s[a] = cp_fmaf(u[1 + a], h2, s[a]);
                }
                float ds[A], tail[T];
                {
                    GradStep<A> g;
                    head.step(s, g2_pick(w4, e), g2_pick(x04, e), g2_pick(x14, e), g);
#pragma unroll
                    for (int a = 0; a < A; ++a) tail[a] = ds[a] = live ? g.ds[a] : 0.0f;
                    tail[A] = live ? g.dls : 0.0f;
#pragma unroll
                    for (int k = 0; k < kGradStats; ++k) tail[A + 1 + k] = live ? g.stat[k] : 0.0f;
                }
#pragma unroll
                for (int d = 0; d < D; ++d) eT[d * kG2Stride + lane] = o[d];
                eT[D * kG2Stride + lane] = 1.0f;
#pragma unroll
                for (int a = 0; a < A; ++a) eT[(D + 1 + a) * kG2Stride + lane] = ds[a];
                // ---- pass 2: the units of layer 2 again, in chunks of 16, each chunk's products after it ----
                float dh1[kMlpMaxHidden], dht[7];
#pragma unroll
                for (int j = 0; j < kMlpMaxHidden; ++j) dh1[j] = 0.0f;
#pragma unroll
                for (int jj = 0; jj < 7; ++jj) dht[jj] = 0.0f;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    if (cc >= tiles2) break;   // wave-uniform
                    const int kend = H2 - 16 * cc < 16 ? H2 - 16 * cc : 16;
                    for (int kk = 0; kk < kend; ++kk) {
                        const Mlp2Ptr u = p + l2 + (16 * cc + kk) * stride;
                        const float pre = pre2_of(u);
                        const float h2 = mlp_activate<ACT>(pre);
                        const float dpre2 = grad2_dh2<A>(u, ds) * grad_dact<ACT>(pre, h2);
                        c1[kk * kG2Stride + lane] = dpre2;
                        c2[kk * kG2Stride + lane] = h2;
#pragma unroll
                        for (int cb = 0; cb < kMlpMaxHidden; cb += 8) {
                            if (cb >= full) break;
#pragma unroll
                            for (int jj = 0; jj < 8; ++jj) dh1[cb + jj] = cp_fmaf(u[kMlp2Head + cb + jj], dpre2, dh1[cb + jj]);
                            MLP2_ORDER();
                        }
#pragma unroll
                        for (int jj = 0; jj < 7; ++jj) {
                            if (jj >= rem) break;
                            dht[jj] = cp_fmaf(u[kMlp2Head + full + jj], dpre2, dht[jj]);
                        }
                    }
                    g2_wave_sync();
#pragma unroll 4
                    for (int b0 = 0; b0 < 16; ++b0) {
                        const float a = c1[rd + 4 * b0], a2 = c2[rd + 4 * b0], be = eT[rd + 4 * b0];
                        accb2[cc] = g2_mfma(a, be, accb2[cc]);
                        acc3[cc] = g2_mfma(a2, be, acc3[cc]);
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
                            if (nt < tiles1) acc2[cc][nt] = g2_mfma(a, h1T[nt * 16 * kG2Stride + rd + 4 * b0], acc2[cc][nt]);   // wave-uniform
                    }
                    g2_wave_sync();
                }
                // ---- layer 1's terms: dpre1 in chunks of 16 units against E; the tail's rows against E's column of ones ----
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    if (cc >= tiles1) break;
#pragma unroll
                    for (int jj = 0; jj < 16; ++jj) {
                        const int j = 16 * cc + jj;
                        if (j < full) c1[jj * kG2Stride + lane] = dh1[j] * grad_dact<ACT>(h1[j], h1[j]);   // (ReLU: h1_j > 0 exactly when pre1_j > 0)
                    }
                    if (cc == (full >> 4)) {
#pragma unroll
                        for (int jj = 0; jj < 7; ++jj) {
                            if (jj >= rem) break;
                            c1[((full & 15) + jj) * kG2Stride + lane] = dht[jj] * grad_dact<ACT>(ht[jj], ht[jj]);
                        }
                    }
                    g2_wave_sync();
#pragma unroll 4
                    for (int b0 = 0; b0 < 16; ++b0) acc1[cc] = g2_mfma(c1[rd + 4 * b0], eT[rd + 4 * b0], acc1[cc]);
                    g2_wave_sync();
                }
                // the tail — db3, the log-sigma sum, the statistics' sums, whose terms may all have one sign — by grad.hip's wave sum (a tree of six f32
                // additions) and then in f64: a chain of 128 f32 additions would spend the statistics' bound
                float mine = 0.0f;
#pragma unroll
                for (int v = 0; v < T; ++v) {
                    const float r = grad_wave_sum(tail[v]);
                    mine = lane == v ? r : mine;
                }
                if (lane < T) tails[wave][lane] += (double)mine;
            }
            // ---- the accumulators into the block's f64 slab, the four waves in wave order.  A tile's word: row 4 kq + i of its rows, column r16 ----
#pragma unroll 1
            for (int wv = 0; wv < kG2Waves; ++wv) {
                if (wave == wv) {
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int u = 16 * cc + 4 * kq + i;   // the unit of layer 2 (acc2, accb2, acc3) or of layer 1 (acc1)
                            if (u < H2) {
#pragma unroll
                                for (int nt = 0; nt < 4; ++nt)
                                    if (16 * nt + r16 < H1) slab[grad2_at_w2(D, H1, u, 16 * nt + r16)] += (double)acc2[cc][nt][i];
                                if (r16 == D) slab[grad2_at_b2(D, H1, H2, u)] += (double)accb2[cc][i];
                                if (r16 > D && r16 <= D + A) slab[grad2_at_w3(D, H1, H2, r16 - D - 1, u)] += (double)acc3[cc][i];
                            }
                            if (u < H1 && r16 <= D) slab[r16 < D ? grad2_at_w1(D, u, r16) : grad2_at_b1(D, H1, u)] += (double)acc1[cc][i];
                        }
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < T)   // db3[0 .. A-1], the log-sigma sum, the five statistics' sums: the four waves' in wave order
        slab[P - A + (int)threadIdx.x] = ((tails[0][threadIdx.x] + tails[1][threadIdx.x]) + tails[2][threadIdx.x]) + tails[3][threadIdx.x];
    __syncthreads();
    double* out = c.workspace + (uint64_t)blockIdx.x * (uint64_t)W;
    for (int i = (int)threadIdx.x; i < W; i += kBlock) out[i] = slab[i];
}

template <int D, int A, int ACT, class Head>
static void launch_form(hipStream_t stream, const GradCall& c, const Mlp2Net<D, A>& net, const Head& head) {
    const bool four = grad_four_per_lane(c, Head::kPpo);
    const int N = four ? 4 : 1;
    const unsigned blocks = grad_blocks(c, N, kG2Steps / N);
    if (four) hipLaunchKernelGGL((grad2_kernel<D, A, ACT, Head, 4>), dim3(blocks), dim3(kBlock), 0, stream, net, head, c);
    else hipLaunchKernelGGL((grad2_kernel<D, A, ACT, Head, 1>), dim3(blocks), dim3(kBlock), 0, stream, net, head, c);
    grad_finish_launch(stream, c, (int)blocks, mlp2_policy_floats(D, A, net.h1, net.h2), std::is_same<Head, PpoGaussian>::value);
}

int grad2_launch(hipStream_t stream, const GradCall& c, int D, int A, int head, const float* pack_dev, int32_t hidden1, int32_t hidden2, int32_t activation) {
    return with_family(D, A, "mgym two-layer gradient call: no kernels for this family", [&](auto d, auto a) {
        const PpoTerms terms{c.lo, c.hi, c.ent_coef};
        with_activation(activation, std::true_type{}, [&](auto act) {
            if (head == GRAD_HEAD_VALUE) launch_form<d.value, 1, act.value>(stream, c, Mlp2Net<d.value, 1>{pack_dev, hidden1, hidden2, 0.0f}, ValueMse{});
            else if constexpr (a.value == 1)
                launch_form<d.value, 1, act.value>(stream, c, Mlp2Net<d.value, 1>{pack_dev, hidden1, hidden2, c.sigma}, PpoGaussian{terms, c.sigma, c.k, c.ent});
            else launch_form<d.value, a.value, act.value>(stream, c, Mlp2Net<d.value, a.value>{pack_dev, hidden1, hidden2, 0.0f}, PpoCategorical<a.value>{terms});
        });
    });
}

}  // namespace mgym
