// The C++ host-side mirror (include/mgym.hpp) with an episode time limit: a MountainCarV0 built with max_episode_steps steps to
// truncation, a LunarLanderV3 likewise, and a VecGym reads the elapsed count back.  Built and run by tests/test_gpu_time_limit.py;
// needs a GPU.
#include <cstdio>
#include <memory>
#include <vector>

#include "../../include/mgym.hpp"

using namespace mgym_host;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    {   // not in the reference (mountain_car.rs:324-329 never truncates): the builder's superset argument
        std::unique_ptr<MountainCarV0> env(MountainCarV0::builder().seed(7).max_episode_steps(6).build());
        REQUIRE(env->reset().size() == 2);
        for (int t = 1; t <= 8; ++t) {
            StepInfo si = env->step(1u);
            REQUIRE(si.reward == -1.0f && !si.done);
            REQUIRE(si.truncated == (t >= 6));   // no auto-reset: past the limit it stays up
        }
        env->reset();
        REQUIRE(!env->step(1u).truncated);
    }
    {
        std::unique_ptr<MountainCarV0> env(MountainCarV0::builder().build());   // the default: off
        env->reset();
        for (int t = 0; t < 300; ++t) REQUIRE(!env->step(1u).truncated);
    }
    {
        std::unique_ptr<LunarLanderV3> env(LunarLanderV3::builder().enable_wind(true).seed(42).max_episode_steps(4).build());
        env->reset();
        for (int t = 1; t <= 5; ++t) REQUIRE(env->step(0u).truncated == (t >= 4));
    }
    {
        mgym_config c;
        check(mgym_default_config(MGYM_MOUNTAINCAR, &c));
        REQUIRE(c.max_episode_steps == 0u);
        c.n_envs = 8; c.flags = MGYM_FLAG_AUTO_RESET; c.max_episode_steps = 3;
        VecGym vec(c);
        REQUIRE(vec.max_episode_steps() == 3u);
        void* p = nullptr;
        check(mgym_malloc(0, 8 * 4, &p)); uint32_t* act = static_cast<uint32_t*>(p);
        check(mgym_malloc(0, 8 * 4, &p)); uint32_t* el = static_cast<uint32_t*>(p);
        check(mgym_malloc(0, 16, &p)); uint8_t* trunc = static_cast<uint8_t*>(p);
        std::vector<uint32_t> h(8, 1u), he(8);
        check(mgym_memcpy_h2d(0, act, h.data(), 32));
        vec.reset();
        for (int t = 1; t <= 7; ++t) {
            vec.step(act, nullptr, nullptr, nullptr, trunc);
            vec.get_elapsed_steps(el);
            vec.sync();
            uint8_t ht[8];
            check(mgym_memcpy_d2h(0, ht, trunc, 8));
            check(mgym_memcpy_d2h(0, he.data(), el, 32));
            for (int i = 0; i < 8; ++i) { REQUIRE(ht[i] == (t % 3 == 0)); REQUIRE(he[i] == (uint32_t)(t % 3)); }
        }
        REQUIRE(vec.episode_count() == 16u);
        c.max_episode_steps = 65536;
        bool threw = false;
        try { VecGym bad(c); } catch (const std::invalid_argument&) { threw = true; }
        REQUIRE(threw);
        mgym_free(0, act); mgym_free(0, el); mgym_free(0, trunc);
    }
    std::printf("time limit mirror ok\n");
    return 0;
}
