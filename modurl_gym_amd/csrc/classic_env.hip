// classic_env.hip — ClassicEnv's allocations and the elapsed-count kernels of mgym_get_elapsed_steps / mgym_set_elapsed_steps.
#include "classic_env.h"
#include "time_limit.h"

namespace mgym {

__global__ void classic_get_elapsed_kernel(const uint16_t* __restrict__ elapsed, uint64_t n, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = elapsed[i];
}

__global__ void classic_set_elapsed_kernel(uint16_t* __restrict__ elapsed, uint64_t n, const uint32_t* __restrict__ in) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) elapsed[i] = (uint16_t)tl_clamp(in[i]);
}

ClassicEnv::~ClassicEnv() {
    if (cols) (void)hipFree(cols);
    if (el_col) (void)hipFree(el_col);
}

int ClassicEnv::alloc(int ncols) {
    MGYM_HIP(hipMalloc(&cols, ncols * n_pad * sizeof(float)));
    MGYM_HIP(hipMemsetAsync(cols, 0, ncols * n_pad * sizeof(float), stream));
    MGYM_HIP(hipMalloc(&el_col, n_pad * sizeof(uint16_t)));
    MGYM_HIP(hipMemsetAsync(el_col, 0, n_pad * sizeof(uint16_t), stream));
    return MGYM_OK;
}

int ClassicEnv::elapsed(uint32_t* out, const uint32_t* in) {
    return out ? launch_per_env(classic_get_elapsed_kernel, el_col, n, out) : launch_per_env(classic_set_elapsed_kernel, el_col, n, in);
}

}  // namespace mgym
