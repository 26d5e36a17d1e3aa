// CPU check of the LunarLander policy header (modurl_gym_amd/csrc/ll_policy.h, compiled for the host through the same shim as ll_host_check.cpp):
// reads cases on stdin, prints the header's actions on stdout.  Built and run by tests/test_ll_policy_host.py, which restates both policies.
//   "L w0 .. w35 o0 .. o7"          -> ll_linear_action (weights and observation as 32-bit patterns in hex)
//   "U seed call g t"               -> ll_uniform_action
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#define __device__
#define __host__
#define __forceinline__ inline
#include "../../modurl_gym_amd/csrc/ll_policy.h"

static float f_of(unsigned long long u) { const uint32_t w = (uint32_t)u; float f; memcpy(&f, &w, 4); return f; }

int main() {
    char kind[4];
    while (scanf("%3s", kind) == 1) {
        if (kind[0] == 'L') {
            mgym::LLLinearPolicy p;
            float o[8];
            unsigned long long u;
            for (int j = 0; j < 4; ++j) {
                for (int c = 0; c < 8; ++c) { if (scanf("%llx", &u) != 1) return 2; p.w[j][c] = f_of(u); }
                if (scanf("%llx", &u) != 1) return 2;
                p.b[j] = f_of(u);
            }
            for (int c = 0; c < 8; ++c) { if (scanf("%llx", &u) != 1) return 2; o[c] = f_of(u); }
            printf("%u\n", mgym::ll_linear_action(p, o));
        } else if (kind[0] == 'U') {
            unsigned long long seed, call, g, t;
            if (scanf("%llu %llu %llu %llu", &seed, &call, &g, &t) != 4) return 2;
            printf("%u\n", mgym::ll_uniform_action(seed, (uint32_t)call, g, (uint32_t)t));
        } else {
            return 2;
        }
    }
    return 0;
}
