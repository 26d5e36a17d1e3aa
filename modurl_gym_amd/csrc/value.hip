// value.hip — mgym_value_mlp (include/mgym.h): a critic's values over a rollout's observation rows, the words of value.h.
//
// Dense pass, one launch: the (K + 1) x n independent evaluations of value_out and last_value_out.  Four-per-lane form (n % 4 == 0 and below 2^30, float
// pointers 16-byte aligned): a lane owns four consecutive environments of one row, loads the row's D components as D 16-byte words, runs
// mlp_scores<D, 1, ACT, 4> — the weights are scalar operands of its packed chains — and stores one 16-byte word.  A row's address is a wave-uniform 64-bit
// base plus the lane's 32-bit byte offset, as in gae.hip; blockIdx.y is the row, so a wave walks one row per weight fetch (rows beyond the grid's 65535 by a
// stride loop).  Otherwise one environment per lane with 64-bit addresses, the same words.
//
// Final pass, a second launch on the same stream where the call has the final triple: its cost follows the number of selected env-steps, not K x n.  A block
// is one wave and owns 256 consecutive environments over kValueChunk steps.  Phase 1 walks the flag rows (4-byte words of four environments where n % 4 == 0
// and the flag pointers are 4-byte aligned, else bytes) and compacts the selected (t, i) by ballot and lane counts into a list in LDS, two bytes an entry.
// Phase 2 evaluates the list 64 entries at a time, one environment per lane: D sparse 4-byte loads of final_obs, mlp_scores<D, 1, ACT, 1>, one 4-byte store.
// No global queue and no atomics: every output word is a pure function of its own inputs, so the list's order reaches no result.  A word of final_obs
// outside the selection is never loaded.
#include "common.h"
#include "value.h"

namespace mgym {

template <class V, class T>
__device__ __forceinline__ V& word_at(T* row, uint32_t off) {
    typedef typename std::conditional<std::is_const<T>::value, const char, char>::type Byte;
    return *reinterpret_cast<V*>(reinterpret_cast<Byte*>(row) + off);
}

template <int D, int ACT, class Net>
__global__ void __launch_bounds__(kBlock) value4_kernel(const Net net, const ValueCall a) {
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;   // (n < 2^30: lanes and byte offsets fit 32 bits)
    if (lane >= (uint32_t)(a.n / 4)) return;
    const uint32_t off16 = lane * 16u;
    for (int32_t r = (int32_t)blockIdx.y; r <= a.K; r += (int32_t)gridDim.y) {   // wave-uniform
        const float* in = value_row_in(r, a.n, D, a.obs_first, a.obs);
        float4 c[D];
#pragma unroll
        for (int q = 0; q < D; ++q) c[q] = word_at<const float4>(in + (uint64_t)q * a.n, off16);
        float o[4][D], s[4][1];
#pragma unroll
        for (int q = 0; q < D; ++q) { o[0][q] = c[q].x; o[1][q] = c[q].y; o[2][q] = c[q].z; o[3][q] = c[q].w; }
        mlp_scores<D, 1, ACT, 4>(net, o, s);
        word_at<float4>(value_row_out(r, a.K, a.n, a.value_out, a.last_value_out), off16) = make_float4(s[0][0], s[1][0], s[2][0], s[3][0]);
    }
}

template <int D, int ACT, class Net>
__global__ void __launch_bounds__(kBlock) value1_kernel(const Net net, const ValueCall a) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    for (int32_t r = (int32_t)blockIdx.y; r <= a.K; r += (int32_t)gridDim.y)
        value_row_out(r, a.K, a.n, a.value_out, a.last_value_out)[i] = value_of<D, ACT>(net, value_row_in(r, a.n, D, a.obs_first, a.obs), a.n, i);
}

// The final pass.  An entry is (step within the chunk) << 8 | (environment within the wave's 256).  words: the flags move as 4-byte words, lane l holding
// environments 4 l .. 4 l + 3 of the wave's; else as bytes, lane l holding environments l, 64 + l, 128 + l, 192 + l.
template <int D, int ACT, class Net>
__global__ void __launch_bounds__(64) value_final_kernel(const Net net, const ValueCall a, const int words) {
    __shared__ uint16_t list[kValueChunk * kValueWaveEnvs];
    const uint32_t l = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kValueWaveEnvs;   // < n
    const int32_t chunks = (a.K + kValueChunk - 1) / kValueChunk;
    for (int32_t ch = (int32_t)blockIdx.y; ch < chunks; ch += (int32_t)gridDim.y) {   // block-uniform
        const int32_t t0 = ch * kValueChunk;
        const int cnt = a.K - t0 < kValueChunk ? a.K - t0 : kValueChunk;
        uint32_t count = 0;   // wave-uniform: entries listed so far, at most 256 x cnt
        for (int b0 = 0; b0 < cnt; b0 += 4) {
            uint32_t sel[4];   // bit j: the lane's j-th environment is selected on step t0 + b0 + b
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                sel[b] = 0u;
                if (b0 + b < cnt) {
                    const uint64_t row = (uint64_t)(t0 + b0 + b) * a.n;
                    if (words) {
                        const uint64_t e = base + 4u * l;   // (n % 4 == 0: the word is inside the row or wholly beyond it)
                        if (e < a.n) {
                            const uint32_t tw = *reinterpret_cast<const uint32_t*>(a.trunc + row + e);
                            const uint32_t dw = a.done ? *reinterpret_cast<const uint32_t*>(a.done + row + e) : 0u;
#pragma unroll
                            for (int j = 0; j < 4; ++j) sel[b] |= (((tw >> (8 * j)) & 0xffu) != 0 && ((dw >> (8 * j)) & 0xffu) == 0) ? 1u << j : 0u;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {   // (both bytes loaded, then one selection: the loads of a step stand together, and no branch nests in a lane's)
                            const uint64_t e = base + 64u * j + l;
                            uint32_t tb = 0u, db = 0u;
                            if (e < a.n) {
                                tb = a.trunc[row + e];
                                db = a.done ? a.done[row + e] : 0u;
                            }
                            sel[b] |= (tb != 0u && db == 0u) ? 1u << j : 0u;
                        }
                    }
                }
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool hit = (sel[b] >> j) & 1u;
                    const uint64_t m = __ballot(hit);
                    const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    if (hit) list[count + before] = (uint16_t)(((b0 + b) << 8) | (words ? 4u * l + j : 64u * j + l));   // count + before < 256 x cnt
                    count += (uint32_t)__popcll(m);
                }
            }
        }
        __syncthreads();   // the block is one wave: the list is complete for every lane
        for (uint32_t k = 0; k < count; k += 64u) {
            if (k + l < count) {
                const uint32_t e = list[k + l];
                const int32_t t = t0 + (int32_t)(e >> 8);              // < K
                const uint64_t i = base + (e & 0xffu);                 // < n: only environments below n are listed
                a.final_value_out[(uint64_t)t * a.n + i] = value_of<D, ACT>(net, a.final_obs + (uint64_t)t * D * a.n, a.n, i);
            }
        }
        __syncthreads();   // the next chunk writes the list again
    }
}

constexpr uint64_t kFourMaxEnvs = 1ull << 30;   // the four-per-lane kernel addresses a row by a 32-bit byte offset
constexpr unsigned kMaxGridY = 65535u;

template <int D, int ACT, class Net>
static void launch_all(hipStream_t stream, const ValueCall& c, const Net& net) {
    const bool four = c.n % 4 == 0 && c.n < kFourMaxEnvs && aligned(c.obs_first, 16) && aligned(c.obs, 16) && aligned(c.value_out, 16) && aligned(c.last_value_out, 16);
    const unsigned rows = (unsigned)c.K + 1u < kMaxGridY ? (unsigned)c.K + 1u : kMaxGridY;
    if (four) hipLaunchKernelGGL((value4_kernel<D, ACT, Net>), dim3((unsigned)((c.n / 4 + kBlock - 1) / kBlock), rows), dim3(kBlock), 0, stream, net, c);
    else hipLaunchKernelGGL((value1_kernel<D, ACT, Net>), dim3((unsigned)((c.n + kBlock - 1) / kBlock), rows), dim3(kBlock), 0, stream, net, c);
    if (c.final_obs) {
        const int words = c.n % 4 == 0 && aligned(c.done, 4) && aligned(c.trunc, 4) ? 1 : 0;   // (a null done is aligned)
        const unsigned chunks = (unsigned)((c.K + kValueChunk - 1) / kValueChunk);
        hipLaunchKernelGGL((value_final_kernel<D, ACT, Net>), dim3((unsigned)((c.n + kValueWaveEnvs - 1) / kValueWaveEnvs), chunks < kMaxGridY ? chunks : kMaxGridY),
                           dim3(64), 0, stream, net, c, words);
    }
}

template <int D>
static void launch_dim(hipStream_t stream, const ValueCall& c, const float* critic, int32_t h1, int32_t h2, int32_t act, const float* pack_dev) {
    if (h2 == 0) {
        static_assert(sizeof(MlpPack<8, 1>) == 2568 && sizeof(MlpPack<8, 1>) + sizeof(ValueCall) + 16 <= 4096, "value kernels: by-value kernel arguments above 4096 bytes");
        MlpPack<D, 1> pack;
        mlp_pack<D, 1>(critic, h1, pack);
        if (act == MLP_ACT_RELU) launch_all<D, MLP_ACT_RELU>(stream, c, pack);
        else if (act == MLP_ACT_TANH) launch_all<D, MLP_ACT_TANH>(stream, c, pack);
        else launch_all<D, MLP_ACT_TANH_FAST>(stream, c, pack);
    } else {
        const Mlp2Net<D, 1> net{pack_dev, h1, h2, 0.0f};
        if (act == MLP_ACT_RELU) launch_all<D, MLP_ACT_RELU>(stream, c, net);
        else launch_all<D, MLP_ACT_TANH_FAST>(stream, c, net);
    }
}

int value_launch(hipStream_t stream, const ValueCall& c, int D, const float* critic, int32_t hidden1, int32_t hidden2, int32_t activation, const float* pack_dev) {
    switch (D) {
    case 2: launch_dim<2>(stream, c, critic, hidden1, hidden2, activation, pack_dev); break;
    case 3: launch_dim<3>(stream, c, critic, hidden1, hidden2, activation, pack_dev); break;
    case 4: launch_dim<4>(stream, c, critic, hidden1, hidden2, activation, pack_dev); break;
    case 6: launch_dim<6>(stream, c, critic, hidden1, hidden2, activation, pack_dev); break;
    case 8: launch_dim<8>(stream, c, critic, hidden1, hidden2, activation, pack_dev); break;
    default: set_last_error("mgym_value_mlp: no kernels for this observation width"); return MGYM_ERR_BAD_ARG;
    }
    MGYM_HIP(hipGetLastError());
    return MGYM_OK;
}

}  // namespace mgym
