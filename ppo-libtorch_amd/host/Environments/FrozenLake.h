// FrozenLake-v1 / FrozenLake8x8-v1 with is_slippery = True (gymnasium's toy_text/frozen_lake.py; the reference has no such env): the host-side class of
// PPO_ENV_FROZENLAKE and PPO_ENV_FROZENLAKE8X8, the CPU twin of the device env.  It computes on the CPU from the same statement -- include/ppo_hip.h: the maps,
// the step, the slip drawn from Philox keyed by state words, the one-hot observation -- in integers, so a state stepped here and by
// ppo_env_transition(PPO_ENV_FROZENLAKE | PPO_ENV_FROZENLAKE8X8, ..) gives the same numbers (tests/test_gpu_frozenlake_facade.py).  It needs no device and no
// library.  The randomness of an episode rides in its state: {cell, j, k0, k1}, the cell, the steps taken and the episode's key.
#pragma once
#include <array>
#include <cstdint>
#include <tuple>
#include <vector>

class FrozenLake {
  public:
    std::vector<float> state;      // {cell, j, k0, k1}: cell in 0..side*side-1 (row-major); j, k0, k1 in 0..2^24-1
    int64_t episode_length;
    float episode_reward;

    // side: 4 (FrozenLake-v1) or 8 (FrozenLake8x8-v1); any other value throws std::invalid_argument
    explicit FrozenLake(int side = 4, int64_t seed = 1, int64_t env_index = 0);
    int side() const { return m_side; }
    // {observation (side*side floats: the one-hot of the cell), reward (0 or 1), terminated, truncated (never: the algorithm counts max_episode_steps)};
    // action in 0..3 (left, down, right, up), clamped
    std::tuple<std::vector<float>, float, bool, bool> step(int64_t action);
    std::vector<float> reset();    // the start cell, no steps taken, a fresh key; the observation of the new state
    std::vector<float> observation() const;

    // the bare step: st[4] (components converted and clamped into their ranges) -> next state in place; returns the reward
    static float transition(int side, float* st, int action, bool& terminated);
    static void observe(int side, const float* st, float* obs);
    static bool isHole(int side, int cell);
    static std::array<uint32_t, 4> philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3);

  private:
    int m_side;
    int64_t m_seed, m_env_index, m_resets = 0;
};
