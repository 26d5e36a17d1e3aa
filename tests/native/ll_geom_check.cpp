// The collision-geometry probe of the LunarLander KERNEL SOURCE on the host: modurl_gym_amd/csrc/ll_geom_probe.h — the per-case
// body of mgym_ll_geom_probe — compiled through the shim of ll_host_check.cpp.  Built and run by tests/test_ll_geom_host.py.
//   ll_geom_check <fn> <count> <in file> <out file>
// fn, columns and words as mgym_ll_geom_probe (include/mgym.h); the files are the raw columns, [cols][count] 32-bit words.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#include "../../modurl_gym_amd/csrc/ll_geom_probe.h"
using namespace mgym;

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: ll_geom_check <fn> <count> <in file> <out file>\n"); return 2; }
    const int fn = atoi(argv[1]);
    const uint64_t count = strtoull(argv[2], nullptr, 0);
    if (fn < 0 || fn >= GEOM_FN_COUNT || count == 0 || (fn == GEOM_SHAPES && count != 1)) { fprintf(stderr, "bad fn or count\n"); return 2; }
    std::vector<float> in((size_t)geom_in_cols(fn) * count + 1), out((size_t)geom_out_cols(fn) * count);
    if (geom_in_cols(fn)) {
        FILE* f = fopen(argv[3], "rb");
        if (!f || fread(in.data(), 4, (size_t)geom_in_cols(fn) * count, f) != (size_t)geom_in_cols(fn) * count) { fprintf(stderr, "short input\n"); return 2; }
        fclose(f);
    }
    LLConst k;
    ll_make_const(k, -10.0f, 0, 15.0f, 1.5f);
    PolyTab tab;  // what stage_tab() copies into LDS on the device
    for (int p = 0; p < 2; ++p) { tab.count[p] = k.poly_count[p]; for (int q = 0; q < kMaxPoly; ++q) { tab.v[p][q] = k.poly_v[p][q]; tab.n[p][q] = k.poly_n[p][q]; } }
    V2 tmp[2 * kMaxPoly];
    for (uint64_t i = 0; i < count; ++i) {
        switch (fn) {
            case GEOM_SHAPES: ll_geom_probe_case<GEOM_SHAPES>(k, tab, tmp, count, i, in.data(), out.data()); break;
            case GEOM_DISTANCE: ll_geom_probe_case<GEOM_DISTANCE>(k, tab, tmp, count, i, in.data(), out.data()); break;
            case GEOM_MANIFOLD: ll_geom_probe_case<GEOM_MANIFOLD>(k, tab, tmp, count, i, in.data(), out.data()); break;
            default: ll_geom_probe_case<GEOM_TOI>(k, tab, tmp, count, i, in.data(), out.data()); break;
        }
    }
    FILE* f = fopen(argv[4], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { fprintf(stderr, "cannot write output\n"); return 2; }
    fclose(f);
    return 0;
}
