// value.hip — mgym_value_mlp (include/mgym.h): a critic's values over a rollout's observation rows, the words of value.h.
//
// Dense pass, one launch: the (K + 1) x n independent evaluations of value_out and last_value_out.  Four-per-lane form (n % 4 == 0 and below 2^30, float
// pointers 16-byte aligned), the dense kernel of learner.h with ValueCall: a lane owns four consecutive environments of one row, loads the row's D components as D 16-byte words, runs
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
#include "learner.h"

namespace mgym {

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

template <int D, int ACT, class Net>
static void launch_all(hipStream_t stream, const ValueCall& c, const Net& net) {
    launch_dense<D, 1, ACT>(stream, c, net, four_per_lane(c.n, c.obs_first, c.obs, c.value_out, c.last_value_out), (unsigned)c.K + 1u, value1_kernel<D, ACT, Net>);
    if (c.final_obs) {
        const int words = c.n % 4 == 0 && aligned(c.done, 4) && aligned(c.trunc, 4) ? 1 : 0;   // (a null done is aligned)
        hipLaunchKernelGGL((value_final_kernel<D, ACT, Net>), dim3((unsigned)((c.n + kValueWaveEnvs - 1) / kValueWaveEnvs), grid_rows((unsigned)((c.K + kValueChunk - 1) / kValueChunk))),
                           dim3(64), 0, stream, net, c, words);
    }
}

int value_launch(hipStream_t stream, const ValueCall& c, int D, const float* critic, int32_t hidden1, int32_t hidden2, int32_t activation, const float* pack_dev) {
    return with_family(D, 0, "mgym_value_mlp: no kernels for this observation width", [&](auto d, auto) {
        with_net<d.value, 1>(critic, hidden1, hidden2, pack_dev, 0.0f, [&](const auto& net, auto two) {
            with_activation(activation, two, [&](auto act) { launch_all<d.value, act.value>(stream, c, net); });
        });
    });
}

}  // namespace mgym
