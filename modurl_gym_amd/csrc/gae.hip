// gae.hip — mgym_gae and mgym_episode_returns (include/mgym.h): one launch each over the rollouts' [K][n_envs] buffers, the chains of gae.h.
//
// Four-per-lane form (n % 4 == 0 and below 2^30, float pointers 16-byte aligned, flag pointers 4-byte aligned): a lane owns four consecutive environments, a
// reward / value / output row moves as one 16-byte word and the four flag bytes of a row as one 4-byte word.  The chain is sequential in t but no load depends
// on it, so the loop takes kGaeBatch steps at a time: every load of the batch is issued, then the batch's arithmetic runs and its stores follow — the latency
// of a row is paid once per batch, not once per step.  K % kGaeBatch steps run first as a partial batch (its slots are guarded by wave-uniform tests).
// final_value and the outputs of mgym_episode_returns are touched only where the flags say so, by 4-byte accesses of the owning lane, issued for the whole
// batch once its flags have arrived.  A row's address is a wave-uniform base (scalar registers) plus the lane's 32-bit byte offset, the same for every row: two
// VGPRs of addresses in all, whatever the batch.  No LDS, no atomics, no cross-lane traffic; the trip count is wave-uniform.
// Otherwise: one environment per lane through gae_env / ep_env, the same words.
#include "common.h"
#include "gae.h"

namespace mgym {

constexpr int B = kGaeBatch;

__device__ __forceinline__ bool flag_of(uint32_t word, int j) { return ((word >> (8 * j)) & 0xffu) != 0; }

// row t of a [K][n] buffer of T (wave-uniform), and the word at a lane's byte offset in it
template <class T>
__device__ __forceinline__ T* row_of(T* base, int32_t t, uint64_t n) { return base + (uint64_t)t * n; }
template <class V, class T>
__device__ __forceinline__ V& at_off(T* row, uint32_t off) {
    typedef typename std::conditional<std::is_const<T>::value, const char, char>::type Byte;
    return *reinterpret_cast<V*>(reinterpret_cast<Byte*>(row) + off);
}

// steps t_top, t_top - 1, .. of the lane's four environments (slot b is step t_top - b); FULL: B of them, else cnt < B.  off16 / off4: the lane's byte offset
// in a row of floats / of flag bytes
template <bool HD, bool HT, bool FV, bool FULL>
__device__ __forceinline__ void gae4_batch(const GaeCall& a, uint32_t off16, uint32_t off4, int32_t t_top, int cnt, GaeChain (&s)[4]) {
    float4 r[B], v[B];
    uint32_t df[B], tf[B];
    float4 fv[B];
    asm volatile("" : "+s"(t_top));   // rows are addressed from t afresh in every batch: as induction variables the 7 x B row pointers do not fit the scalar registers
#pragma unroll
    for (int b = 0; b < B; ++b) {
        if (FULL || b < cnt) {
            const int32_t t = t_top - b;
            r[b] = at_off<const float4>(row_of(a.reward, t, a.n), off16);
            v[b] = at_off<const float4>(row_of(a.value, t, a.n), off16);
            df[b] = HD ? at_off<const uint32_t>(row_of(a.done, t, a.n), off4) : 0u;
            tf[b] = HT ? at_off<const uint32_t>(row_of(a.trunc, t, a.n), off4) : 0u;
        }
    }
    // final_value: the lane's 16-byte word of a row, loaded only by a lane that has an environment truncated and not terminated on that step (the other three
    // words come with it and are never selected: a memory sector costs the same either way)
#pragma unroll
    for (int b = 0; b < B; ++b) {
        if (FULL || b < cnt) {
            bool need = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) need |= flag_of(tf[b], j) && !flag_of(df[b], j);
            fv[b] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (FV && need) fv[b] = at_off<const float4>(row_of(a.final_value, t_top - b, a.n), off16);
        }
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
        if (FULL || b < cnt) {
            const int32_t t = t_top - b;
            const float rr[4] = {r[b].x, r[b].y, r[b].z, r[b].w}, vv[4] = {v[b].x, v[b].y, v[b].z, v[b].w}, ff[4] = {fv[b].x, fv[b].y, fv[b].z, fv[b].w};
            float adv[4], ret[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) gae_link(a.gamma, a.gl, rr[j], vv[j], flag_of(df[b], j), flag_of(tf[b], j), ff[j], s[j], adv[j], ret[j]);
            if (a.adv_out) at_off<float4>(row_of(a.adv_out, t, a.n), off16) = make_float4(adv[0], adv[1], adv[2], adv[3]);
            if (a.ret_out) at_off<float4>(row_of(a.ret_out, t, a.n), off16) = make_float4(ret[0], ret[1], ret[2], ret[3]);
            __builtin_amdgcn_sched_barrier(0);   // one step's flag tests at a time: hoisted together, the batch's lane masks do not fit the scalar registers
        }
    }
}

template <bool HD, bool HT, bool FV>
__global__ void __launch_bounds__(kBlock) gae4_kernel(GaeCall a) {
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;   // (n < 2^30: lanes and byte offsets fit 32 bits)
    if (lane >= (uint32_t)(a.n / 4)) return;
    const uint32_t off16 = lane * 16u, off4 = lane * 4u;
    const float4 lv = at_off<const float4>(a.last_value, off16);
    GaeChain s[4] = {{0.0f, lv.x}, {0.0f, lv.y}, {0.0f, lv.z}, {0.0f, lv.w}};
    int32_t t = a.K - 1;
    const int rem = a.K % B;
    if (rem) {
        gae4_batch<HD, HT, FV, false>(a, off16, off4, t, rem, s);
        t -= rem;
    }
    for (; t >= 0; t -= B) gae4_batch<HD, HT, FV, true>(a, off16, off4, t, B, s);
}

__global__ void __launch_bounds__(kBlock) gae1_kernel(GaeCall a) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    gae_env(a.K, a.n, i, a.reward, a.done, a.trunc, a.value, a.last_value, a.final_value, a.gamma, a.gl, a.adv_out, a.ret_out);
}

// steps t0, t0 + 1, .. of the lane's four environments (slot b is step t0 + b)
template <bool HD, bool HT, bool FULL>
__device__ __forceinline__ void ep4_batch(const EpCall& a, uint32_t off16, uint32_t off4, int32_t t0, int cnt, EpChain (&s)[4]) {
    float4 r[B];
    uint32_t df[B], tf[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        if (FULL || b < cnt) {
            r[b] = at_off<const float4>(row_of(a.reward, t0 + b, a.n), off16);
            df[b] = HD ? at_off<const uint32_t>(row_of(a.done, t0 + b, a.n), off4) : 0u;
            tf[b] = HT ? at_off<const uint32_t>(row_of(a.trunc, t0 + b, a.n), off4) : 0u;
        }
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
        if (FULL || b < cnt) {
            const float rr[4] = {r[b].x, r[b].y, r[b].z, r[b].w};
            const uint32_t fin = df[b] | tf[b];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float ret;
                uint32_t len;
                if (ep_link(rr[j], flag_of(fin, j), s[j], ret, len)) {
                    if (a.return_out) at_off<float>(row_of(a.return_out, t0 + b, a.n), off16 + 4 * j) = ret;
                    if (a.length_out) at_off<uint32_t>(row_of(a.length_out, t0 + b, a.n), off16 + 4 * j) = len;
                }
            }
        }
    }
}

template <bool HD, bool HT>
__global__ void __launch_bounds__(kBlock) ep4_kernel(EpCall a) {
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
    if (lane >= (uint32_t)(a.n / 4)) return;
    const uint32_t off16 = lane * 16u, off4 = lane * 4u;
    const float4 acc = at_off<const float4>(a.ep_return, off16);
    const uint4 len = at_off<const uint4>(a.ep_length, off16);
    EpChain s[4] = {{acc.x, len.x}, {acc.y, len.y}, {acc.z, len.z}, {acc.w, len.w}};
    int32_t t = 0;
    for (; t + B <= a.K; t += B) ep4_batch<HD, HT, true>(a, off16, off4, t, B, s);
    if (t < a.K) ep4_batch<HD, HT, false>(a, off16, off4, t, a.K - t, s);
    at_off<float4>(a.ep_return, off16) = make_float4(s[0].acc, s[1].acc, s[2].acc, s[3].acc);
    at_off<uint4>(a.ep_length, off16) = make_uint4(s[0].len, s[1].len, s[2].len, s[3].len);
}

__global__ void __launch_bounds__(kBlock) ep1_kernel(EpCall a) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    ep_env(a.K, a.n, i, a.reward, a.done, a.trunc, a.ep_return, a.ep_length, a.return_out, a.length_out);
}

// one block per 256 lanes, no grid-stride: a lane's whole work is its own chain
static dim3 blocks_for(uint64_t lanes) { return dim3((unsigned)((lanes + kBlock - 1) / kBlock)); }
constexpr uint64_t kFourMaxEnvs = 1ull << 30;   // the four-per-lane kernels address a row by a 32-bit byte offset

int gae_launch(hipStream_t stream, const GaeCall& c) {
    const bool four = c.n % 4 == 0 && c.n < kFourMaxEnvs && aligned(c.reward, 16) && aligned(c.value, 16) && aligned(c.last_value, 16) && aligned(c.adv_out, 16) &&
                      aligned(c.ret_out, 16) && aligned(c.done, 4) && aligned(c.trunc, 4) && aligned(c.final_value, 16);   // (a null pointer is aligned)
    if (four) {
        with_bools([&](auto hd, auto ht, auto fv) {
            hipLaunchKernelGGL((gae4_kernel<decltype(hd)::value, decltype(ht)::value, decltype(fv)::value>), blocks_for(c.n / 4), dim3(kBlock), 0, stream, c);
        }, c.done != nullptr, c.trunc != nullptr, c.final_value != nullptr);
    } else {
        hipLaunchKernelGGL(gae1_kernel, blocks_for(c.n), dim3(kBlock), 0, stream, c);
    }
    MGYM_HIP(hipGetLastError());
    return MGYM_OK;
}

int episode_returns_launch(hipStream_t stream, const EpCall& c) {
    const bool four = c.n % 4 == 0 && c.n < kFourMaxEnvs && aligned(c.reward, 16) && aligned(c.ep_return, 16) && aligned(c.ep_length, 16) && aligned(c.done, 4) &&
                      aligned(c.trunc, 4);   // (return_out / length_out are written by 4-byte stores)
    if (four) {
        with_bools([&](auto hd, auto ht) {
            hipLaunchKernelGGL((ep4_kernel<decltype(hd)::value, decltype(ht)::value>), blocks_for(c.n / 4), dim3(kBlock), 0, stream, c);
        }, c.done != nullptr, c.trunc != nullptr);
    } else {
        hipLaunchKernelGGL(ep1_kernel, blocks_for(c.n), dim3(kBlock), 0, stream, c);
    }
    MGYM_HIP(hipGetLastError());
    return MGYM_OK;
}

}  // namespace mgym
