// CPU check of the MLP policy header (modurl_gym_amd/csrc/mlp_policy.h, the lines the rollout kernels compile), built with g++ -ffp-contract=off.
//   as a program (tests/test_mlp_policy_host.py): cases on stdin, one per line, floats as 32-bit patterns in hex
//       "D A cont act H  <H (D + 1) + A (H + 1) policy words, nn.Linear order>  <D observation words>"
//     -> one line "action s_0 .. s_{A-1}" (hex words; cont = 1: the action word is the bits of s_0)
//   as a shared object (tests/test_gpu_mlp_policy.py): mlp_policy_eval over n environments of an SoA observation
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../modurl_gym_amd/csrc/mlp_policy.h"

using namespace mgym;

template <int D, int A, int ACT, bool CONT>
static void eval(const float* policy, int H, const float* obs, uint64_t n, uint64_t stride, uint32_t* actions, float* scores) {
    MlpPack<D, A> p;
    mlp_pack<D, A>(policy, H, p);
    for (uint64_t i = 0; i < n; ++i) {
        float o[1][D], s[1][A];
        uint32_t a[1];
        for (int q = 0; q < D; ++q) o[0][q] = obs[(uint64_t)q * stride + i];
        mlp_actions<D, A, ACT, CONT, 1>(p, o, a);
        actions[i] = a[0];
        if (scores) {
            mlp_scores<D, A, ACT, 1>(p, o, s);
            for (int k = 0; k < A; ++k) scores[i * A + k] = s[0][k];
        }
    }
}

template <int D, int A, bool CONT>
static int eval_act(int act, const float* policy, int H, const float* obs, uint64_t n, uint64_t stride, uint32_t* actions, float* scores) {
    if (act == MLP_ACT_RELU) eval<D, A, MLP_ACT_RELU, CONT>(policy, H, obs, n, stride, actions, scores);
    else if (act == MLP_ACT_TANH) eval<D, A, MLP_ACT_TANH, CONT>(policy, H, obs, n, stride, actions, scores);
    else return 1;
    return 0;
}

// obs: [D][stride] floats; actions: [n] words; scores: [n][A] floats or NULL.  Returns 0, or 1 for a (D, A, cont, act, H) no family has.
extern "C" int mlp_policy_eval(int D, int A, int cont, int act, int H, const float* policy, const float* obs, uint64_t n, uint64_t stride,
                               uint32_t* actions, float* scores) {
    if (H < 1 || H > kMlpMaxHidden) return 1;
    if (D == 4 && A == 2 && !cont) return eval_act<4, 2, false>(act, policy, H, obs, n, stride, actions, scores);
    if (D == 2 && A == 3 && !cont) return eval_act<2, 3, false>(act, policy, H, obs, n, stride, actions, scores);
    if (D == 2 && A == 1 && cont) return eval_act<2, 1, true>(act, policy, H, obs, n, stride, actions, scores);
    if (D == 8 && A == 4 && !cont) return eval_act<8, 4, false>(act, policy, H, obs, n, stride, actions, scores);
    return 1;
}

static bool rd(float& f) {
    unsigned long long u;
    if (scanf("%llx", &u) != 1) return false;
    const uint32_t w = (uint32_t)u;
    memcpy(&f, &w, 4);
    return true;
}

int main() {
    int D, A, cont, act, H;
    while (scanf("%d %d %d %d %d", &D, &A, &cont, &act, &H) == 5) {
        if (D < 1 || D > 8 || A < 1 || A > 4 || H < 1 || H > kMlpMaxHidden) return 2;
        std::vector<float> pol(mlp_policy_floats(D, A, H));
        float o[8], s[4];
        uint32_t a;
        for (float& v : pol) if (!rd(v)) return 2;
        for (int q = 0; q < D; ++q) if (!rd(o[q])) return 2;
        if (mlp_policy_eval(D, A, cont, act, H, pol.data(), o, 1, 1, &a, s)) return 2;
        printf("%x", a);
        for (int k = 0; k < A; ++k) { uint32_t w; memcpy(&w, &s[k], 4); printf(" %x", w); }
        printf("\n");
    }
    return 0;
}
