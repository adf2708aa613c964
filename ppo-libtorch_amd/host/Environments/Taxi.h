// Taxi-v3 (gymnasium's toy_text/taxi.py, no rain, no fickle passenger; the reference has no such env): the host-side class of PPO_ENV_TAXI, the CPU twin of
// the device env.  It computes on the CPU from the same table -- include/ppo_hip.h: stands, walls, step, mask, the one-hot observation -- in integers, so a
// state stepped here and by ppo_env_transition(PPO_ENV_TAXI, ..) gives the same numbers (tests/test_gpu_taxi_facade.py).  It needs no device and no library.
#pragma once
#include <array>
#include <cstdint>
#include <tuple>
#include <vector>

class Taxi {
  public:
    std::vector<float> state;      // {row, col, pass, dest}: row, col in 0..4; pass in 0..4 (0..3 waiting at R, G, Y, B; 4 in the taxi); dest in 0..3
    int64_t episode_length;
    float episode_reward;

    explicit Taxi(int64_t seed = 1, int64_t env_index = 0);
    // {observation (19 floats: one-hot row, col, pass, dest), reward (-1, -10 or +20), terminated, truncated (never: the algorithm counts max_episode_steps)};
    // action in 0..5 (south, north, east, west, pickup, dropoff), clamped
    std::tuple<std::vector<float>, float, bool, bool> step(int64_t action);
    std::vector<float> reset();    // one of the 300 start states (passenger waiting, not at the destination); the observation of the new state
    std::vector<float> observation() const;
    std::array<uint8_t, 6> actionMask() const;

    // the bare table: st[4] (components converted and clamped into their ranges) -> next state in place; returns the reward
    static float transition(float* st, int action, bool& terminated);
    static void observe(const float* st, float* obs19);
    static std::array<uint8_t, 6> mask(const float* st);
    static void stateOf(const float* obs19, float* st);   // the index of the largest entry of each group, the first on ties

  private:
    int64_t m_seed, m_env_index, m_resets = 0;
};
