// gae.h — the two per-environment scans of mgym_gae and mgym_episode_returns (include/mgym.h), shared by the kernels of gae.hip (four environments per lane,
// or one) and the host check tests/native/gae_check.cpp, which compiles this header with g++ (mgym_math.h's MG_HD is empty there).  Compile with
// -ffp-contract=off: the only fused operations are the two cp_fmaf of a GAE link.
//
//   mgym_gae, t = K-1 down to 0, from carry = +0, nxt = last_value[i]:
//     fin = d | u;  nv = fin ? (d ? +0 : fv) : nxt;  c = fin ? +0 : carry
//     delta = fmaf(gamma, nv, r) - v;  adv = fmaf(gl, c, delta);  ret = adv + v;  carry = adv;  nxt = v
//   mgym_episode_returns, t = 0 .. K-1, from the caller's (acc, len):
//     acc = acc + r;  len = len + 1;  where fin: emit (acc, len), then acc = +0, len = 0
//
// Every ?: is a selection: the word that is not selected (a NaN final_value, the carry across an episode end) is never an operand of any arithmetic.
#pragma once
#include <stdint.h>
#include "mgym_math.h"

namespace mgym {

// Steps whose loads the four-per-lane kernels issue before the arithmetic of the first of them (gae.hip).  8 steps of mgym_gae hold 8 x (4 reward + 4 value +
// 2 flag words) = 80 VGPRs of loaded data, + 32 where final_value is read: 92 .. 137 VGPRs, 3 .. 5 waves per SIMD, no private segment
// (profiles/gae_kernel_resources.txt) — 1 Mi environments are 4 waves per SIMD, and 16 steps would need more than 200 VGPRs.
constexpr int kGaeBatch = 8;

struct GaeChain {
    float carry, nxt;   // adv[t + 1] and V of the observation held after step t, as far as step t may see them
};

// one link of the reverse chain: step t of one environment.  fv is final_value[t][i], or +0 where the caller passed none; it is read only if u && !d
MG_HD void gae_link(float gamma, float gl, float r, float v, bool d, bool u, float fv, GaeChain& s, float& adv, float& ret) {
    const bool fin = d | u;
    const float nv = fin ? (d ? 0.0f : fv) : s.nxt;
    const float c = fin ? 0.0f : s.carry;
    const float delta = cp_fmaf(gamma, nv, r) - v;
    adv = cp_fmaf(gl, c, delta);
    ret = adv + v;
    s.carry = adv;
    s.nxt = v;
}

// environment i of [K][n] buffers, the whole chain (the one-environment-per-lane kernel and the host check); done / trunc / final_value and either output may be null
MG_HD void gae_env(int32_t K, uint64_t n, uint64_t i, const float* reward, const uint8_t* done, const uint8_t* trunc, const float* value, const float* last_value,
                   const float* final_value, float gamma, float gl, float* adv_out, float* ret_out) {
    GaeChain s{0.0f, last_value[i]};
    for (int32_t t = K - 1; t >= 0; --t) {
        const uint64_t at = (uint64_t)t * n + i;
        const bool d = done && done[at] != 0, u = trunc && trunc[at] != 0;
        const float fv = (final_value && u && !d) ? final_value[at] : 0.0f;
        float adv, ret;
        gae_link(gamma, gl, reward[at], value[at], d, u, fv, s, adv, ret);
        if (adv_out) adv_out[at] = adv;
        if (ret_out) ret_out[at] = ret;
    }
}

struct EpChain {
    float acc;      // the running episode's return so far
    uint32_t len;   // ... and its length
};

// one link of the forward chain; true where the episode ended on this step: (ret, len) are then the finished episode's, and the chain starts afresh
MG_HD bool ep_link(float r, bool fin, EpChain& s, float& ret, uint32_t& len) {
    s.acc = s.acc + r;
    s.len = s.len + 1u;
    ret = s.acc;
    len = s.len;
    if (fin) {
        s.acc = 0.0f;
        s.len = 0u;
    }
    return fin;
}

MG_HD void ep_env(int32_t K, uint64_t n, uint64_t i, const float* reward, const uint8_t* done, const uint8_t* trunc, float* ep_return, uint32_t* ep_length,
                  float* return_out, uint32_t* length_out) {
    EpChain s{ep_return[i], ep_length[i]};
    for (int32_t t = 0; t < K; ++t) {
        const uint64_t at = (uint64_t)t * n + i;
        const bool fin = (done && done[at] != 0) || (trunc && trunc[at] != 0);
        float ret;
        uint32_t len;
        if (ep_link(reward[at], fin, s, ret, len)) {
            if (return_out) return_out[at] = ret;
            if (length_out) length_out[at] = len;
        }
    }
    ep_return[i] = s.acc;
    ep_length[i] = s.len;
}

#if defined(__HIPCC__)
// gae.hip: the launches of the two entry points on `stream`, arguments already checked (abi.hip); n > 0, K >= 1
struct GaeCall {
    uint64_t n;
    int32_t K;
    const float* reward;
    const uint8_t *done, *trunc;
    const float *value, *last_value, *final_value;
    float gamma, gl;
    float *adv_out, *ret_out;
};
struct EpCall {
    uint64_t n;
    int32_t K;
    const float* reward;
    const uint8_t *done, *trunc;
    float* ep_return;
    uint32_t* ep_length;
    float* return_out;
    uint32_t* length_out;
};
int gae_launch(hipStream_t stream, const GaeCall& call);
int episode_returns_launch(hipStream_t stream, const EpCall& call);
#endif

}  // namespace mgym
