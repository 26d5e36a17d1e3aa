// tools/cartpole_tune.hip — stand-alone timing harness of the CartPole step kernel's launch forms (NOT product code).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -mllvm -amdgpu-kernarg-preload-count=14 tools/cartpole_tune.hip -o tools/cartpole_tune
// Run:   tools/cartpole_tune [n_envs = 1048576] [graph replays per timing = 50] [block cap of the grid-stride form = 256]
// Times, as 16-step graphs over a ring of 16 action columns: a copy kernel with the step's traffic and no arithmetic (the ceiling), the
// single-pass form at 64 / 128 / 256 threads per block, and the grid-stride form at the given block cap.
#include "../modurl_gym_amd/csrc/cartpole.hip"
#include <vector>
#include <stdio.h>
namespace mgym {
void set_last_error(const std::string& m) { fprintf(stderr, "%s\n", m.c_str()); }
int hip_fail(hipError_t e, const char* what, const char*, int) { fprintf(stderr, "HIP %d %s\n", (int)e, what); return 4; }
Env* make_mountaincar(bool) { return nullptr; }
Env* make_lunarlander() { return nullptr; }

// ceiling: same traffic, no arithmetic
__global__ void __launch_bounds__(kBlock) copy_kernel(CartPoleDev d, const uint32_t* act, float* rew, uint8_t* dn, uint8_t* tr) {
    uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t i0 = g * 4;
    if (i0 >= d.n) return;
    float4 vx = *(const float4*)(d.x() + i0), vxd = *(const float4*)(d.xd() + i0), vth = *(const float4*)(d.th() + i0), vthd = *(const float4*)(d.thd() + i0);
    uint4 vc = *(const uint4*)(d.ctr() + i0), va = *(const uint4*)(act + i0);
    vx.x += 1.f; vxd.y += 1.f; vth.z += 1.f; vthd.w += 1.f; vc.x += va.x;
    *(float4*)(d.x() + i0) = vx; *(float4*)(d.xd() + i0) = vxd; *(float4*)(d.th() + i0) = vth; *(float4*)(d.thd() + i0) = vthd; *(uint4*)(d.ctr() + i0) = vc;
    *(float4*)(rew + i0) = vx; *(uint32_t*)(dn + i0) = vc.y; *(uint32_t*)(tr + i0) = vc.z;
}
}  // namespace mgym
using namespace mgym;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

// one launch of cartpole_step_kernel<4, euler, plain reward, auto-reset, BLK, ONE> with the kernel's flat argument list
template <int BLK, bool ONE>
static void launch_step(CartPoleEnv& env, unsigned blocks, const uint32_t* act, float* rew, uint8_t* dn, uint8_t* tr) {
    const CartPoleDev& d = env.dev;
    hipLaunchKernelGGL((cartpole_step_kernel<4, true, false, true, BLK, ONE>), dim3(blocks), dim3(BLK), 0, env.stream, d.base, (uint32_t)d.n_pad, (uint32_t)d.n, act, d.seed,
                       d.env_id_base, d.err, d.done_count, (float*)nullptr, rew, dn, tr);
}

int main(int argc, char** argv) {
    const uint64_t n = argc > 1 ? strtoull(argv[1], 0, 0) : (1u << 20);
    const int reps = argc > 2 ? atoi(argv[2]) : 50;
    const unsigned cap = argc > 3 ? (unsigned)atoi(argv[3]) : 256u;
    if (n == 0 || n % 1024 || n > (1ull << 23) || cap == 0) { printf("n_envs: a multiple of 1024, at most 8 Mi (one block per tile at every block size); cap >= 1\n"); return 1; }
    CartPoleEnv env; env.cfg.struct_size = sizeof(mgym_config); env.cfg.flags = MGYM_FLAG_AUTO_RESET; env.cfg.is_euler = 1; env.cfg.seed = 1;
    env.n = n; env.n_pad = round_up(n, 1024);
    CK(hipStreamCreate(&env.stream));
    CK(hipMalloc((void**)&env.d_err, 4)); CK(hipMemset(env.d_err, 0, 4));
    CK(hipMalloc((void**)&env.d_done, kDoneShards * sizeof(unsigned long long))); CK(hipMemset(env.d_done, 0, kDoneShards * sizeof(unsigned long long)));
    if (env.init() != MGYM_OK) return 1;
    const int RING = 16;
    uint32_t* act; float* rew; uint8_t *dn, *tr;
    CK(hipMalloc((void**)&act, RING * n * 4)); CK(hipMalloc((void**)&rew, n * 4)); CK(hipMalloc((void**)&dn, n)); CK(hipMalloc((void**)&tr, n));
    { std::vector<uint32_t> h(RING * n); uint32_t s = 12345; for (auto& v : h) { s = s * 1664525u + 1013904223u; v = (s >> 16) & 1; } CK(hipMemcpy(act, h.data(), h.size() * 4, hipMemcpyHostToDevice)); }
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto timeit = [&](const char* name, auto launch) {
        env.reset(nullptr, nullptr, true, nullptr);
        hipGraph_t g; hipGraphExec_t ge;
        CK(hipStreamBeginCapture(env.stream, hipStreamCaptureModeThreadLocal));
        for (int k = 0; k < RING; ++k) launch(act + (uint64_t)k * n);
        CK(hipStreamEndCapture(env.stream, &g)); CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        for (int w = 0; w < 5; ++w) CK(hipGraphLaunch(ge, env.stream));
        CK(hipStreamSynchronize(env.stream));
        float best = 1e9, tot = 0;
        for (int rnd = 0; rnd < 5; ++rnd) {
            CK(hipEventRecord(e0, env.stream));
            for (int r = 0; r < reps; ++r) CK(hipGraphLaunch(ge, env.stream));
            CK(hipEventRecord(e1, env.stream)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= (reps * RING); tot += ms; if (ms < best) best = ms;
        }
        printf("%-36s n=%llu  %.2f us/step (best %.2f)  %.0f GB/s alg  %.3e steps/s\n", name, (unsigned long long)n, tot / 5 * 1e3, best * 1e3, 50.0 * n / (tot / 5 * 1e-3) / 1e9, n / (tot / 5 * 1e-3));
        CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g));
    };
    const unsigned tiles = (unsigned)(n / 1024);
    timeit("copy ceiling (no math)", [&](uint32_t* a) { hipLaunchKernelGGL(copy_kernel, dim3(tiles), dim3(256), 0, env.stream, env.dev, a, rew, dn, tr); });
    timeit("single pass, 64 threads", [&](uint32_t* a) { launch_step<64, true>(env, tiles * 4, a, rew, dn, tr); });
    timeit("single pass, 128 threads", [&](uint32_t* a) { launch_step<128, true>(env, tiles * 2, a, rew, dn, tr); });
    timeit("single pass, 256 threads", [&](uint32_t* a) { launch_step<256, true>(env, tiles, a, rew, dn, tr); });
    if (cap < tiles) timeit("grid stride, 256 threads, capped", [&](uint32_t* a) { launch_step<256, false>(env, cap, a, rew, dn, tr); });
    timeit("copy ceiling again (no math)", [&](uint32_t* a) { hipLaunchKernelGGL(copy_kernel, dim3(tiles), dim3(256), 0, env.stream, env.dev, a, rew, dn, tr); });
    CK(hipStreamSynchronize(env.stream));
    return 0;
}
