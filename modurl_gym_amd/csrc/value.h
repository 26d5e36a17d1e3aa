// value.h — the row mapping and the selection of mgym_value_mlp (include/mgym.h), shared by the kernels of value.hip (four environments per lane, or one) and
// the host check tests/native/value_check.cpp, which compiles this header with g++ (mgym_math.h's MG_HD is empty there).  Compile with -ffp-contract=off: the
// only fused operations are the cp_fmaf of the policy headers' chains.
//
//   V(o) = the one score s_0 of mlp_scores<D, 1, ACT, N> under the critic (mlp_policy.h's MlpPack<D, 1>, or mlp2_policy.h's Mlp2Net<D, 1>): no arithmetic of its own
//   dense rows r = 0 .. K:   input  row r = r == 0 ? obs_first : obs[r - 1]          ([D][n] each)
//                            output row r = r <  K ? value_out[r] : last_value_out   ([n] each)
//   final values:            final_value_out[t][i] = V(final_obs[t][:, i])  exactly where  trunc[t][i] != 0 && (done == NULL || done[t][i] == 0)
// The selection is the one gae.h's gae_env makes (u && !d): a word of final_obs outside it is never loaded, a word of final_value_out outside it never stored.
#pragma once
#include <stdint.h>
#include "mlp2_policy.h"

namespace mgym {

// Steps of one block of the final pass (value.hip): a wave lists the selected env-steps of its 256 environments over this many steps in LDS — 256 x 16 two-byte
// entries, 8 KiB — and then evaluates the list 64 entries at a time.
constexpr int kValueChunk = 16;
constexpr int kValueWaveEnvs = 256;

// dense row r of 0 .. K: the [D][n] observation row it reads and the [n] row it writes
MG_HD const float* value_row_in(int32_t r, uint64_t n, int D, const float* obs_first, const float* obs) {
    return r == 0 ? obs_first : obs + (uint64_t)(r - 1) * (uint64_t)D * n;
}
MG_HD float* value_row_out(int32_t r, int32_t K, uint64_t n, float* value_out, float* last_value_out) { return r < K ? value_out + (uint64_t)r * n : last_value_out; }

// does env-step `at` = t * n + i get a final value: truncated and not terminated (done may be null = all 0)
MG_HD bool value_final_selected(const uint8_t* done, const uint8_t* trunc, uint64_t at) { return trunc[at] != 0 && (!done || done[at] == 0); }

// V of environment i of one [D][n] observation row
template <int D, int ACT, class Net>
MG_HD float value_of(const Net& net, const float* row, uint64_t n, uint64_t i) {
    float o[1][D], s[1][1];
#pragma unroll
    for (int q = 0; q < D; ++q) o[0][q] = row[(uint64_t)q * n + i];
    mlp_scores<D, 1, ACT, 1>(net, o, s);
    return s[0][0];
}

// environment i, every word the call writes for it (the one-environment-per-lane form and the host check); final_obs / final_value_out / trunc all null or
// all set, done may be null
template <int D, int ACT, class Net>
MG_HD void value_env(const Net& net, int32_t K, uint64_t n, uint64_t i, const float* obs_first, const float* obs, const float* final_obs, const uint8_t* done,
                     const uint8_t* trunc, float* value_out, float* last_value_out, float* final_value_out) {
    for (int32_t r = 0; r <= K; ++r) value_row_out(r, K, n, value_out, last_value_out)[i] = value_of<D, ACT>(net, value_row_in(r, n, D, obs_first, obs), n, i);
    if (!final_obs) return;
    for (int32_t t = 0; t < K; ++t) {
        const uint64_t at = (uint64_t)t * n + i;
        if (value_final_selected(done, trunc, at)) final_value_out[at] = value_of<D, ACT>(net, final_obs + (uint64_t)t * D * n, n, i);
    }
}

#if defined(__HIPCC__)
// value.hip: the launches of mgym_value_mlp on `stream`, arguments already checked (abi.hip); n > 0, K >= 1.  `critic`: the caller's host words; hidden2 == 0:
// they travel by value as an MlpPack<D, 1>, else `pack_dev` (the handle's second weight pack) holds them by then (Env::mlp2_store_to)
struct ValueCall {
    uint64_t n;
    int32_t K;
    const float *obs_first, *obs, *final_obs;
    const uint8_t *done, *trunc;
    float *value_out, *last_value_out, *final_value_out;
    // what learner.h's dense kernel asks of a call: rows 0 .. K, no action row, the one score
    static constexpr bool kActions = false;
    __device__ __forceinline__ int32_t rows() const { return K + 1; }
    __device__ __forceinline__ float* out_row(int32_t r) const { return value_row_out(r, K, n, value_out, last_value_out); }
    template <int A> __device__ __forceinline__ float word(const float (&s)[A], uint32_t) const { return s[0]; }
};
int value_launch(hipStream_t stream, const ValueCall& call, int D, const float* critic, int32_t hidden1, int32_t hidden2, int32_t activation, const float* pack_dev);
#endif

}  // namespace mgym
