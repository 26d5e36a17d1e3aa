// selftest.hip — on-device proof that the cheap CartPole instruction sequences (cartpole_math.h / cartpole_step.h)
// equal the reference-form arithmetic ON THE SILICON THAT RUNS THEM (hardware v_rcp_f32, v_fma_f32/f64, v_div_*):
// the same enumerations as tests/native/cartpole_fast_check.cpp, evaluated by gfx950 kernels.
//   out[0] sincos : every f32 with |y| < 0.75, both signs       cp_sincos_small == mg_sincosf
//   out[1] divc   : every f32 in the proven range               cp_div_const(x, 1.1f) == x / 1.1f  (IEEE v_div_* sequence)
//   out[2] div    : every f32 cos value c in [0, 1] -> divisor d, 32 numerators each (random + hard cases)
//   out[3] step   : 2^28 random guard-admitted states, all four <EULER, SB> variants: fast form == reference form
//   out[4] sincos_u : every f32 with |y| < 120, both signs: the fused lock-step mg_sincosf_u / mg_cosf_u (LunarLander,
//                   MountainCar) == mg_sincosf / mg_cosf
// Exposed as mgym_selftest_cartpole_math() (test seam; seconds on an MI355X).  mgym_math_probe() (test seam) writes the device's
// result bits of one mgym_math.h entry point for a span of input patterns; tests/test_gpu_math_exhaustive.py compares all 2^32 with glibc.
// mgym_ll_geom_probe() (test seam) runs LunarLander's collision-geometry primitives (ll_b2.h: b2Distance, b2TimeOfImpact,
// b2CollideEdgeAndPolygon + b2WorldManifold, the polygon tables and mass data) as pure functions, one case per lane;
// tests/test_gpu_ll_geom.py checks them against a float64 reference and, word for word, against the oracle and the host build.
#include "common.h"
#include "cartpole_step.h"
#include "ll_kernel_common.h"
#include "ll_geom_probe.h"
#include "mlp_policy.h"

namespace mgym {

__device__ __forceinline__ uint32_t st_lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s; }
__device__ __forceinline__ float st_rnd_float(uint32_t& s, uint32_t lo_e, uint32_t hi_e) {
    const uint32_t b = st_lcg(s), e = lo_e + (st_lcg(s) >> 8) % (hi_e - lo_e + 1u);
    return as_f32((b & 0x807fffffu) | (e << 23));
}

__device__ __forceinline__ void st_flush(unsigned long long* out, unsigned long long bad) {
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_down(bad, o);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(out, bad);
}

__global__ void __launch_bounds__(256) selftest_sincos_kernel(unsigned long long* out) {
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < 0x3f400000ull; u += stride) {
#pragma unroll
        for (uint32_t sg = 0; sg < 2; ++sg) {
            const float y = as_f32((uint32_t)u | (sg << 31));
            float s0, c0, s1, c1;
            mg_sincosf(y, &s0, &c0);
            cp_sincos_small(y, &s1, &c1);
            bad += (as_u32(s0) != as_u32(s1) || as_u32(c0) != as_u32(c1)) ? 1u : 0u;
        }
    }
    st_flush(out, bad);
}

__global__ void __launch_bounds__(256) selftest_sincos_u_kernel(unsigned long long* out) {
    unsigned long long bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < 0x42f00000ull; u += stride) {
#pragma unroll
        for (uint32_t sg = 0; sg < 2; ++sg) {
            const float y = as_f32((uint32_t)u | (sg << 31));
            float s0, c0, s1, c1;
            mg_sincosf(y, &s0, &c0);
            mg_sincosf_u(y, &s1, &c1);
            const float c2 = mg_cosf_u(y);
            bad += (as_u32(s0) != as_u32(s1) || as_u32(c0) != as_u32(c1) || as_u32(c2) != as_u32(c0)) ? 1u : 0u;
        }
    }
    st_flush(out, bad);
}

__global__ void __launch_bounds__(256) selftest_divc_kernel(unsigned long long* out) {
    unsigned long long bad = 0;
    constexpr CartPoleParams P = cartpole_params(1, 0);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < 0x100000000ull; u += stride) {
        const float x = as_f32((uint32_t)u);
        if (!cp_div_range_ok(x)) continue;
        // volatile copy: keeps the compiler from folding x / const into a reciprocal multiply of its own choosing
        volatile float m = P.total_mass;
        const float ref = x / m, got = cp_div_const(x, P.total_mass, P.inv_total_mass);
        bad += as_u32(ref) != as_u32(got) ? 1u : 0u;
    }
    st_flush(out, bad);
}

__global__ void __launch_bounds__(256) selftest_div_kernel(unsigned long long* out) {
    unsigned long long bad = 0;
    constexpr CartPoleParams P = cartpole_params(1, 0);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u <= 0x3f800000ull; u += stride) {
        const float c = as_f32((uint32_t)u);
        const float d = P.length * (4.0f / 3.0f - P.masspole * c * c / P.total_mass);  // cartpole.rs:269-270
        uint32_t rng = (uint32_t)u * 0x9E3779B9u + 12345u;
        for (int k = 0; k < 32; ++k) {
            const uint32_t bits = st_lcg(rng), e8 = 27u + (st_lcg(rng) >> 8) % 200u;  // 2^-100 .. 2^99
            float n = as_f32((bits & 0x807fffffu) | (e8 << 23));
            if (k == 0) n = 0.0f;
            if (k == 1) n = -0.0f;
            if (k == 2) n = d;
            if (k == 3) n = d * 3.0f;
            if (k == 4) n = as_f32(as_u32(d) + 1u);
            if (k == 5) n = -as_f32(as_u32(d) - 1u);
            const float ref = n / d, got = cp_div(n, d);
            bad += as_u32(ref) != as_u32(got) ? 1u : 0u;
        }
    }
    st_flush(out, bad);
}

template <bool EULER, bool SB>
__device__ __forceinline__ unsigned long long selftest_step_group(uint32_t seed, int count) {
    constexpr CartPoleParams P = cartpole_params(EULER ? 1 : 0, SB ? 1 : 0);
    unsigned long long bad = 0;
    uint32_t s = seed;
    for (int it = 0; it < count; ++it) {
        float x, xd, th, thd;
        const uint32_t mode = st_lcg(s) >> 29;
        if (mode < 5) {
            x = ((int32_t)st_lcg(s)) * (3.0f / 2147483648.0f); xd = ((int32_t)st_lcg(s)) * (4.0f / 2147483648.0f);
            th = ((int32_t)st_lcg(s)) * (0.3f / 2147483648.0f); thd = ((int32_t)st_lcg(s)) * (4.0f / 2147483648.0f);
        } else {
            x = st_rnd_float(s, 0, 200); xd = st_rnd_float(s, 0, 200);
            th = st_rnd_float(s, 0, 126); thd = st_rnd_float(s, 0, 166);
            if ((st_lcg(s) >> 30) == 0) th = as_f32(st_lcg(s) & 0x80000000u);
            if ((st_lcg(s) >> 30) == 0) thd = as_f32(st_lcg(s) & 0x80000000u);
        }
        const uint32_t action = st_lcg(s) >> 31;
        uint32_t ctr = cp_ctr_pack((st_lcg(s) >> 8) % 1030u, st_lcg(s) >> 30, st_lcg(s));
        if ((st_lcg(s) >> 28) == 0) ctr = (ctr & ~kCpStepsMask) | (498u + (st_lcg(s) >> 30));
        if (!cartpole_fast_ok(th, thd, action)) continue;
        float a0 = x, a1 = xd, a2 = th, a3 = thd, b0 = x, b1 = xd, b2 = th, b3 = thd, ra, rb;
        uint32_t ca = ctr, cb = ctr, da, ta, db, tb;
        cartpole_step_ref(P, a0, a1, a2, a3, ca, action, ra, da, ta);
        cartpole_step_fast<EULER, SB>(P, b0, b1, b2, b3, cb, action, rb, db, tb);
        const bool same = ca == cb && da == db && ta == tb && as_u32(ra) == as_u32(rb) && as_u32(a0) == as_u32(b0) &&
                          as_u32(a1) == as_u32(b1) && as_u32(a2) == as_u32(b2) && as_u32(a3) == as_u32(b3);
        bad += same ? 0u : 1u;
    }
    return bad;
}

__global__ void __launch_bounds__(256) selftest_step_kernel(unsigned long long* out, int per_thread) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bad = 0;
    bad += selftest_step_group<true, false>(0x1234567u + tid * 2654435761u, per_thread);
    bad += selftest_step_group<true, true>(0x2345678u + tid * 2654435761u, per_thread / 4);
    bad += selftest_step_group<false, false>(0x3456789u + tid * 2654435761u, per_thread / 4);
    bad += selftest_step_group<false, true>(0x456789au + tid * 2654435761u, per_thread / 4);
    st_flush(out, bad);
}

// result bits of one mgym_math.h entry point for the patterns first .. first + count - 1 (mgym_math_probe); the sincos
// forms write sin to out[i] and cos to out[count + i]
template <int FN>
__global__ void __launch_bounds__(256) math_probe_kernel(uint32_t first, uint64_t count, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const float y = as_f32(first + (uint32_t)i);
        if constexpr (FN == MGYM_MATH_SINCOSF || FN == MGYM_MATH_SINCOSF_U) {
            float s, c;
            if constexpr (FN == MGYM_MATH_SINCOSF) mg_sincosf(y, &s, &c);
            else mg_sincosf_u(y, &s, &c);
            out[i] = as_u32(s);
            out[count + i] = as_u32(c);
        } else {
            float r;
            if constexpr (FN == MGYM_MATH_SINF) r = mg_sinf(y);
            else if constexpr (FN == MGYM_MATH_COSF) r = mg_cosf(y);
            else if constexpr (FN == MGYM_MATH_COSF_U) r = mg_cosf_u(y);
            else r = mg_tanhf(y);
            out[i] = as_u32(r);
        }
    }
}

// result bits of mlp_policy.h's hidden activation for the patterns first .. first + count - 1 (mgym_act_probe)
template <int ACT>
__global__ void __launch_bounds__(256) act_probe_kernel(uint32_t first, uint64_t count, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) out[i] = as_u32(mlp_activate<ACT>(as_f32(first + (uint32_t)i)));
}

// mlp_policy.h's draw for one case per lane (mgym_sample_probe): scores [A][count], one Philox word per case; the action, and c_0 .. c_{A-1} if asked
template <int A>
__global__ void __launch_bounds__(256) sample_probe_kernel(uint64_t count, const float* __restrict__ scores, const uint32_t* __restrict__ words, uint32_t* __restrict__ actions,
                                                           float* __restrict__ cum) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        float s[A], c[A];
#pragma unroll
        for (int a = 0; a < A; ++a) s[a] = scores[(uint64_t)a * count + i];
        actions[i] = mlp_sample<A>(s, words[i]);
        if (cum) {
            mlp_sample_cum<A>(s, c);
#pragma unroll
            for (int a = 0; a < A; ++a) cum[(uint64_t)a * count + i] = c[a];
        }
    }
}

// mlp_policy.h's Box-Muller pair for one pair of Philox words per lane (mgym_gauss_probe): the two normals, and q = -2 ln(u1) as an f32 if asked
__global__ void __launch_bounds__(256) gauss_probe_kernel(uint64_t count, const uint32_t* __restrict__ wa, const uint32_t* __restrict__ wb, float* __restrict__ z_even,
                                                          float* __restrict__ z_odd, float* __restrict__ q) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        float ze, zo;
        mlp_gauss_pair(wa[i], wb[i], &ze, &zo);
        z_even[i] = ze;
        z_odd[i] = zo;
        if (q) q[i] = mlp_gauss_q(wa[i]);
    }
}

// one case per lane (ll_geom_probe.h).  As in every product kernel the polygon table and collide_edge_polygon's per-lane buffer are
// LDS: that function casts both to the LDS address space.
constexpr int kGeomBlock = 64;
template <int FN>
__global__ void __launch_bounds__(kGeomBlock) ll_geom_probe_kernel(LLConst k, uint64_t count, const float* __restrict__ in, float* __restrict__ out) {
    __shared__ PolyTab tab;
    __shared__ V2 s_tmp[kGeomBlock * 2 * kMaxPoly];
    stage_tab(tab, k);
    const uint64_t i = (uint64_t)blockIdx.x * kGeomBlock + threadIdx.x;
    if (i >= count) return;  // ragged tail (past the barrier of stage_tab)
    ll_geom_probe_case<FN>(k, tab, s_tmp + threadIdx.x * (2 * kMaxPoly), count, i, in, out);
}

}  // namespace mgym

using namespace mgym;

static_assert(MGYM_LL_GEOM_SHAPES == GEOM_SHAPES && MGYM_LL_GEOM_DISTANCE == GEOM_DISTANCE && MGYM_LL_GEOM_MANIFOLD == GEOM_MANIFOLD &&
              MGYM_LL_GEOM_TOI == GEOM_TOI, "mgym.h and ll_geom_probe.h number the probes alike");

extern "C" int mgym_ll_geom_probe(int device, int fn, uint64_t count, const float* in, float* out) {
    const bool shapes = fn == MGYM_LL_GEOM_SHAPES;
    if (fn < MGYM_LL_GEOM_SHAPES || fn > MGYM_LL_GEOM_TOI || !out || (!shapes && !in) || count == 0 || count > (1ull << 31) || (shapes && count != 1)) {
        set_last_error("mgym_ll_geom_probe: unknown probe, NULL columns, or a case count of 0, above 2^31 or (SHAPES) other than 1");
        return MGYM_ERR_BAD_ARG;
    }
    LLConst k;
    ll_make_const(k, -10.0f, 0, 15.0f, 1.5f);
    int prev = -1;
    (void)hipGetDevice(&prev);
    MGYM_HIP(hipSetDevice(device));
    const dim3 grid((unsigned)((count + kGeomBlock - 1) / kGeomBlock)), block(kGeomBlock);
    switch (fn) {
        case MGYM_LL_GEOM_SHAPES: hipLaunchKernelGGL(ll_geom_probe_kernel<GEOM_SHAPES>, grid, block, 0, nullptr, k, count, in, out); break;
        case MGYM_LL_GEOM_DISTANCE: hipLaunchKernelGGL(ll_geom_probe_kernel<GEOM_DISTANCE>, grid, block, 0, nullptr, k, count, in, out); break;
        case MGYM_LL_GEOM_MANIFOLD: hipLaunchKernelGGL(ll_geom_probe_kernel<GEOM_MANIFOLD>, grid, block, 0, nullptr, k, count, in, out); break;
        default: hipLaunchKernelGGL(ll_geom_probe_kernel<GEOM_TOI>, grid, block, 0, nullptr, k, count, in, out); break;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (prev >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) return hip_fail(e, "ll_geom_probe", __FILE__, __LINE__);
    return MGYM_OK;
}

extern "C" int mgym_sample_probe(int device, int32_t n_actions, uint64_t count, const float* scores, const uint32_t* words, uint32_t* actions_out, float* cum_out) {
    if (n_actions < 2 || n_actions > 4 || count == 0 || count > (1ull << 31) || !scores || !words || !actions_out) {
        set_last_error("mgym_sample_probe: n_actions outside 2 .. 4, a case count of 0 or above 2^31, or NULL scores, words or actions_out");
        return MGYM_ERR_BAD_ARG;
    }
    int prev = -1;
    (void)hipGetDevice(&prev);
    MGYM_HIP(hipSetDevice(device));
    const uint64_t blocks = (count + 255) / 256;
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536)), block(256);
    switch (n_actions) {
        case 2: hipLaunchKernelGGL(sample_probe_kernel<2>, grid, block, 0, nullptr, count, scores, words, actions_out, cum_out); break;
        case 3: hipLaunchKernelGGL(sample_probe_kernel<3>, grid, block, 0, nullptr, count, scores, words, actions_out, cum_out); break;
        default: hipLaunchKernelGGL(sample_probe_kernel<4>, grid, block, 0, nullptr, count, scores, words, actions_out, cum_out); break;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (prev >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) return hip_fail(e, "sample_probe", __FILE__, __LINE__);
    return MGYM_OK;
}

extern "C" int mgym_gauss_probe(int device, uint64_t count, const uint32_t* wa, const uint32_t* wb, float* z_even_out, float* z_odd_out, float* q_out) {
    if (count == 0 || count > (1ull << 31) || !wa || !wb || !z_even_out || !z_odd_out) {
        set_last_error("mgym_gauss_probe: a case count of 0 or above 2^31, or NULL wa, wb, z_even_out or z_odd_out");
        return MGYM_ERR_BAD_ARG;
    }
    int prev = -1;
    (void)hipGetDevice(&prev);
    MGYM_HIP(hipSetDevice(device));
    const uint64_t blocks = (count + 255) / 256;
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536)), block(256);
    hipLaunchKernelGGL(gauss_probe_kernel, grid, block, 0, nullptr, count, wa, wb, z_even_out, z_odd_out, q_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (prev >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) return hip_fail(e, "gauss_probe", __FILE__, __LINE__);
    return MGYM_OK;
}

extern "C" int mgym_math_probe(int device, int fn, uint32_t first, uint64_t count, uint32_t* out) {
    if (!out || count == 0 || count > 0x100000000ull - first || fn < MGYM_MATH_SINF || fn > MGYM_MATH_TANHF) {
        set_last_error("mgym_math_probe: NULL output, empty or out-of-range pattern span, or unknown entry point");
        return MGYM_ERR_BAD_ARG;
    }
    int prev = -1;
    (void)hipGetDevice(&prev);
    MGYM_HIP(hipSetDevice(device));
    const uint64_t blocks = (count + 255) / 256;
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536)), block(256);
    switch (fn) {
        case MGYM_MATH_SINF: hipLaunchKernelGGL(math_probe_kernel<MGYM_MATH_SINF>, grid, block, 0, nullptr, first, count, out); break;
        case MGYM_MATH_COSF: hipLaunchKernelGGL(math_probe_kernel<MGYM_MATH_COSF>, grid, block, 0, nullptr, first, count, out); break;
        case MGYM_MATH_SINCOSF: hipLaunchKernelGGL(math_probe_kernel<MGYM_MATH_SINCOSF>, grid, block, 0, nullptr, first, count, out); break;
        case MGYM_MATH_SINCOSF_U: hipLaunchKernelGGL(math_probe_kernel<MGYM_MATH_SINCOSF_U>, grid, block, 0, nullptr, first, count, out); break;
        case MGYM_MATH_COSF_U: hipLaunchKernelGGL(math_probe_kernel<MGYM_MATH_COSF_U>, grid, block, 0, nullptr, first, count, out); break;
        default: hipLaunchKernelGGL(math_probe_kernel<MGYM_MATH_TANHF>, grid, block, 0, nullptr, first, count, out); break;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (prev >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) return hip_fail(e, "math_probe", __FILE__, __LINE__);
    return MGYM_OK;
}

extern "C" int mgym_act_probe(int device, int activation, uint32_t first, uint64_t count, uint32_t* out) {
    if (!out || count == 0 || count > 0x100000000ull - first || (activation != MGYM_ACT_RELU && activation != MGYM_ACT_TANH && activation != MGYM_ACT_TANH_FAST)) {
        set_last_error("mgym_act_probe: NULL output, empty or out-of-range pattern span, or unknown activation");
        return MGYM_ERR_BAD_ARG;
    }
    int prev = -1;
    (void)hipGetDevice(&prev);
    MGYM_HIP(hipSetDevice(device));
    const uint64_t blocks = (count + 255) / 256;
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536)), block(256);
    switch (activation) {
        case MGYM_ACT_RELU: hipLaunchKernelGGL(act_probe_kernel<MLP_ACT_RELU>, grid, block, 0, nullptr, first, count, out); break;
        case MGYM_ACT_TANH: hipLaunchKernelGGL(act_probe_kernel<MLP_ACT_TANH>, grid, block, 0, nullptr, first, count, out); break;
        default: hipLaunchKernelGGL(act_probe_kernel<MLP_ACT_TANH_FAST>, grid, block, 0, nullptr, first, count, out); break;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (prev >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) return hip_fail(e, "act_probe", __FILE__, __LINE__);
    return MGYM_OK;
}

extern "C" int mgym_selftest_cartpole_math(int device, uint64_t* mismatches /* [5] */) {
    if (!mismatches) { set_last_error("mgym_selftest_cartpole_math: NULL"); return MGYM_ERR_BAD_ARG; }
    int prev = -1;
    (void)hipGetDevice(&prev);
    MGYM_HIP(hipSetDevice(device));
    unsigned long long* d = nullptr;
    MGYM_HIP(hipMalloc((void**)&d, 5 * sizeof(unsigned long long)));
    MGYM_HIP(hipMemset(d, 0, 5 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(selftest_sincos_kernel, dim3(4096), dim3(256), 0, nullptr, d + 0);
    hipLaunchKernelGGL(selftest_divc_kernel, dim3(4096), dim3(256), 0, nullptr, d + 1);
    hipLaunchKernelGGL(selftest_div_kernel, dim3(4096), dim3(256), 0, nullptr, d + 2);
    hipLaunchKernelGGL(selftest_step_kernel, dim3(4096), dim3(256), 0, nullptr, d + 3, 160);
    hipLaunchKernelGGL(selftest_sincos_u_kernel, dim3(4096), dim3(256), 0, nullptr, d + 4);
    hipError_t e = hipDeviceSynchronize();
    unsigned long long h[5] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (prev >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) return hip_fail(e, "selftest", __FILE__, __LINE__);
    for (int i = 0; i < 5; ++i) mismatches[i] = h[i];
    return MGYM_OK;
}
