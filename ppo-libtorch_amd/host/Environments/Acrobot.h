// Acrobot-v1 (gymnasium's classic_control/acrobot.py, "book" dynamics, no torque noise; the reference has no such env): the host-side class of
// PPO_ENV_ACROBOT.  Unlike the other host env classes it computes on the CPU: the step is the library's arithmetic written out -- include/ppo_hip.h's
// formulas in the same f32 association, glibc's sinf / cosf (which the device functions reproduce bit for bit) and the same large-argument rule -- so a state
// stepped here and by ppo_env_transition(PPO_ENV_ACROBOT, ..) gives the same bits (tests/test_gpu_acrobot_facade.py).  It needs no device and no library.
// Build it with floating-point contraction off (-ffp-contract=off), as the library is.
#pragma once
#include <cstdint>
#include <tuple>
#include <vector>

class Acrobot {
  public:
    std::vector<float> state;      // {theta1, theta2, w1, w2}
    int64_t episode_length;
    float episode_reward;

    explicit Acrobot(int64_t seed = 1, int64_t env_index = 0);
    // {observation (cos th1, sin th1, cos th2, sin th2, w1, w2), reward (-1, or 0 on the terminating step), terminated, truncated (never: the algorithm counts
    // max_episode_steps)}; action in {0, 1, 2}: torque action - 1
    std::tuple<std::vector<float>, float, bool, bool> step(int64_t action);
    std::vector<float> reset();    // four values in [-0.1, 0.1); the observation of the new state
    std::vector<float> observation() const;

    // the bare arithmetic: st[4] -> next state in place; returns the reward
    static float transition(float* st, int action, bool& terminated);
    static void observe(const float* st, float* obs6);
    static float sinr(float x);    // sinf with the header's large-argument rule
    static float cosr(float x);

  private:
    int64_t m_seed, m_env_index, m_resets = 0;
};
